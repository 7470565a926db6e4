"""BEV rendering, the host half (pointnet_refine_amd.bev) and the g13 fixture the reference's viewer
produced: the colour table, the PNG writer, the zoom rule, the maximum-per-pixel rule pinned to the
reference's images on the CPU, the overlay oracle on hand-checked pixels, and the no-fallback rule."""
import json
import os
import struct
import zlib

import numpy as np
import pytest
import torch

import _bev_oracle as O


def load_g13(golden_dir):
    z = dict(np.load(os.path.join(golden_dir, "g13_bev.npz")))
    z["names"] = json.loads(bytes(z["names"]).decode())
    return z


def max_per_pixel(pts, res, pad, extent=None):
    """generate_bev_map as a maximum: numpy in the dtype of the points, one rounding per operation."""
    T = pts.dtype.type
    x, y, inten = pts[:, 0], pts[:, 1], pts[:, 3].astype(np.float32)
    if extent is None:
        x_min, x_max, y_min, y_max = x.min() - T(pad), x.max() + T(pad), y.min() - T(pad), y.max() + T(pad)
    else:
        y_min, y_max, x_min, x_max = (T(e) for e in extent)
    w, h = int((y_max - y_min) / T(res)), int((x_max - x_min) / T(res))
    u, v = ((y - y_min) / T(res)).astype(np.int32), ((x_max - x) / T(res)).astype(np.int32)
    ok = (u >= 0) & (u < w) & (v >= 0) & (v < h)
    best = np.full(h * w, -np.inf, dtype=np.float32)
    np.maximum.at(best, v[ok].astype(np.int64) * w + u[ok], inten[ok])
    return np.where(np.isinf(best), np.float32(0), best).reshape(h, w), [y_min, y_max, x_min, x_max]


def read_png(path):
    """Decodes an 8-bit RGBA PNG whose rows use filter 0; verifies every CRC."""
    raw = open(path, "rb").read()
    assert raw[:8] == b"\x89PNG\r\n\x1a\n"
    pos, chunks = 8, []
    while pos < len(raw):
        n, kind = struct.unpack(">I4s", raw[pos:pos + 8])
        data = raw[pos + 8:pos + 8 + n]
        assert struct.unpack(">I", raw[pos + 8 + n:pos + 12 + n])[0] == zlib.crc32(kind + data) & 0xffffffff
        chunks.append((kind, data))
        pos += 12 + n
    assert [k for k, _ in chunks][0] == b"IHDR" and chunks[-1] == (b"IEND", b"")
    w, h, depth, colour, comp, filt, lace = struct.unpack(">IIBBBBB", chunks[0][1])
    assert (depth, colour, comp, filt, lace) == (8, 6, 0, 0, 0)
    rows = np.frombuffer(zlib.decompress(b"".join(d for k, d in chunks if k == b"IDAT")), dtype=np.uint8)
    rows = rows.reshape(h, 1 + 4 * w)
    assert np.all(rows[:, 0] == 0)
    return rows[:, 1:].reshape(h, w, 4).copy()


def test_jet_table_is_matplotlibs(golden_dir):
    from pointnet_refine_amd import bev
    z = load_g13(golden_dir)
    assert np.array_equal(bev.jet_table(), z["jet"])
    g = bev.gray_table()
    assert g.shape == (256, 4) and np.array_equal(g[:, 0], np.arange(256)) and np.all(g[:, 3] == 255)


@pytest.mark.parametrize("shape", [(7, 5), (1, 1)])
def test_write_png_round_trip(tmp_path, shape):
    from pointnet_refine_amd import bev
    img = np.random.default_rng(3).integers(0, 256, shape + (4,)).astype(np.uint8)
    path = str(tmp_path / "a.png")
    bev.write_png(path, img)
    assert np.array_equal(read_png(path), img)
    bev.write_png(path, torch.from_numpy(img))
    assert np.array_equal(read_png(path), img)
    with pytest.raises(ValueError):
        bev.write_png(path, img[..., :3])


def test_item_windows_match_reference(golden_dir):
    from pointnet_refine_amd import bev
    z = load_g13(golden_dir)
    items = json.loads(bytes(z["win_items"]).decode())
    wins, kept = bev.item_windows(items)
    assert kept == z["win_kept"].tolist() and len(kept) < len(items)
    assert np.array_equal(wins, z["win_windows"])
    # the same items as io.load_scene_items gives them
    arr = lambda l: np.array([[p["x"], p["y"], p["z"]] for p in l], dtype=np.float64).reshape(-1, 3)
    loaded = [{"position": arr(it["position"]) if "position" in it else None,
               "noisy_candidates": [arr(c) for c in it.get("noisy_candidates", [])]} for it in items]
    wins2, kept2 = bev.item_windows(loaded)
    assert kept2 == kept and np.array_equal(wins2, wins)


def test_fixture_images_are_the_maximum_per_pixel(golden_dir):
    z = load_g13(golden_dir)
    assert len(z["names"]) >= 7
    for k, name in enumerate(z["names"]):
        pts = z[f"c{k}_pts"]
        img, ext = max_per_pixel(pts, float(z[f"c{k}_res"]), float(z[f"c{k}_pad"]))
        want = z[f"c{k}_image"]
        assert img.shape == want.shape and np.array_equal(img, want), name
        assert z[f"c{k}_extent"].dtype == pts.dtype and np.array_equal(np.array(ext, dtype=pts.dtype), z[f"c{k}_extent"])
    k = z["names"].index("negative")
    assert (z[f"c{k}_image"] < 0).any()                        # a pixel of negative intensities only stays negative


def test_overlay_oracle_hand_checked_pixels():
    canvas = np.zeros((12, 20, 4), dtype=np.uint8)
    canvas[..., 3] = 255
    win, res = [0.0, 20.0, 0.0, 12.0], 1.0                     # pixel units are metres here
    st = {"color": (0, 255, 0), "width": 2.0, "alpha": 1.0, "dash": None}
    # a horizontal line along v = 6 (x = 12 - 6) from u = 2 to u = 18: rows 5 and 6 have centres 0.5 away
    out, touched = O.draw(canvas, win, [np.array([[6.0, 2.0], [6.0, 18.0]])], [st], res)
    assert out[5, 10].tolist() == [0, 255, 0, 255] and out[6, 10].tolist() == [0, 255, 0, 255]   # d = 0.5: c = 1
    assert out[4, 10].tolist() == [0, 0, 0, 255] and out[7, 10].tolist() == [0, 0, 0, 255]       # d = 1.5: c = 0
    assert not touched[4, 10] and touched[5, 10]
    assert out[5, 1].tolist()[1] == round(255 * (1.5 - np.hypot(0.5, 0.5)))                       # the end cap
    half = dict(st, width=1.0, alpha=0.5)
    out, _ = O.draw(canvas, win, [np.array([[6.0, 2.0], [6.0, 18.0]])], [half], res)
    assert out[5, 10, 1] == 64 and out[6, 10, 1] == 64         # c = 0.5 + 0.5 - 0.5, times alpha 0.5: 63.75 -> 64
    # dashed, 4 on / 3 off from the first vertex at u = 2: on [2, 6), off [6, 9), on [9, 13)
    dashed = dict(st, dash=(4.0, 3.0))
    out, touched = O.draw(canvas, win, [np.array([[6.0, 2.0], [6.0, 18.0]])], [dashed], res)
    assert touched[5, 3] and touched[5, 5] and not touched[5, 6] and not touched[5, 8] and touched[5, 9]
    assert touched[5, 12] and not touched[5, 13]
    # two lines: the later one is composited over the earlier one
    red = {"color": (255, 0, 0), "width": 2.0, "alpha": 0.5, "dash": None}
    out, _ = O.draw(canvas, win, [np.array([[6.0, 2.0], [6.0, 18.0]]), np.array([[2.0, 10.0], [10.0, 10.0]])], [st, red], res)
    assert out[5, 10].tolist() == [128, 128, 0, 255] and out[5, 5].tolist() == [0, 255, 0, 255]


@pytest.mark.skipif(torch.cuda.is_available(), reason="checks the no-GPU behaviour")
def test_gpu_functions_raise_without_a_gpu():
    from pointnet_refine_amd import bev
    pts = np.zeros((4, 4), dtype=np.float32)
    img = np.zeros((4, 4), dtype=np.float32)
    rgba = np.zeros((4, 4, 4), dtype=np.uint8)
    for call in (lambda: bev.bev_map(pts), lambda: bev.tone_map(img), lambda: bev.tone_map(torch.from_numpy(img)),
                 lambda: bev.draw_lines(torch.from_numpy(rgba), [0, 1, 0, 1], [], [], []),
                 lambda: bev.crop_views(torch.from_numpy(rgba), [0, 1, 0, 1], [[0, 1, 0, 1]]),
                 lambda: bev.render_scene(None, pts, []), lambda: bev.bev_maps(pts, [0, 4], [0, 1, 0, 1]),
                 lambda: bev.colorize(img, img), lambda: bev.chamfer_xy([pts], [pts])):
        with pytest.raises(RuntimeError):
            call()


def test_package_imports_no_plotting_library():
    src = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "pointnet_refine_amd", "bev.py")).read()
    for name in ("matplotlib", "PIL", "scipy", "oracle"):
        assert f"import {name}" not in src and f"from {name}" not in src
