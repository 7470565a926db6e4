"""BEV rendering on the GPU (csrc/prh_bev.hpp through pointnet_refine_amd.bev) against the g13
fixture the reference's viewer produced, the numpy maximum-per-pixel of test_bev_cpu.py and the
brute-force overlay oracle of _bev_oracle.py.  Pixels of the intensity image and colours are
exact; p within 1 float32 ulp where numpy interpolates; norm within rtol 1e-6; overlays within 1
per channel, untouched pixels exactly untouched."""
import json
import os

import numpy as np
import pytest
import torch

import _bev_oracle as O
import test_bev_cpu as R

pytestmark = pytest.mark.gpu


def _bev():
    from pointnet_refine_amd import bev
    return bev


def _clouds(z):
    for k, name in enumerate(z["names"]):
        yield k, name, z[f"c{k}_pts"], float(z[f"c{k}_res"]), float(z[f"c{k}_pad"])


def test_bev_map_equals_reference_pixel_for_pixel(golden_dir):
    B = _bev()
    z = R.load_g13(golden_dir)
    dtypes = set()
    for k, name, pts, res, pad in _clouds(z):
        img, ext = B.bev_map(pts, res, pad)
        want = z[f"c{k}_image"]
        assert img.dtype == torch.float32 and tuple(img.shape) == want.shape, name
        got = img.cpu().numpy()
        assert np.array_equal(got, want), (name, int((got != want).sum()))
        assert all(type(e) == pts.dtype.type for e in ext)
        assert np.array_equal(np.array(ext, dtype=pts.dtype), z[f"c{k}_extent"]), name
        img2, ext2 = B.bev_map(torch.from_numpy(pts).cuda(), res, pad)
        assert torch.equal(img, img2) and ext == ext2
        assert torch.equal(img, B.bev_map(pts, res, pad)[0])
        # extra columns are ignored; a given extent reproduces the image
        wide = np.column_stack([pts, np.full(len(pts), 9.0, dtype=pts.dtype)])
        assert torch.equal(img, B.bev_map(wide, res, pad)[0])
        assert torch.equal(img, B.bev_map(pts, res, extent=ext)[0])
        dtypes.add(pts.dtype)
    assert dtypes == {np.dtype(np.float32), np.dtype(np.float64)}


def test_bev_map_rejects_bad_input():
    B = _bev()
    pts = np.random.default_rng(0).uniform(0, 5, (100, 4)).astype(np.float32)
    for col, val in ((0, np.nan), (1, np.inf), (3, -np.inf), (3, np.nan)):
        bad = pts.copy()
        bad[17, col] = val
        with pytest.raises(ValueError):
            B.bev_map(bad)
        with pytest.raises(ValueError):
            B.bev_map(bad.astype(np.float64), extent=[-5, 10, -5, 10])
    with pytest.raises(ValueError):
        B.bev_map(np.zeros((0, 4), dtype=np.float32))
    with pytest.raises(ValueError):
        B.bev_map(pts.astype(np.float16))
    with pytest.raises(RuntimeError):
        B.bev_map(torch.from_numpy(pts))


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_bev_map_at_size(dtype):
    B = _bev()
    rng = np.random.default_rng(21)
    n = 2_000_000
    pts = np.column_stack([rng.uniform(-30, 30, n), rng.uniform(-25, 25, n), rng.normal(0, 0.2, n),
                           rng.integers(0, 65536, n)]).astype(dtype)
    want, ext_want = R.max_per_pixel(pts, 0.05, 5.0)
    img, ext = B.bev_map(pts)
    got = img.cpu().numpy()
    assert got.shape == want.shape and np.array_equal(got, want), int((got != want).sum())
    assert [float(e) for e in ext] == [float(e) for e in ext_want]
    assert torch.equal(img, B.bev_map(pts)[0])


def test_bev_maps_equals_bev_map_per_slice(golden_dir):
    B = _bev()
    from pointnet_refine_amd import drive as D
    z = np.load(os.path.join(golden_dir, "g11_drive_slices.npz"))
    cloud, poses = np.ascontiguousarray(z["d0_cloud"], dtype=np.float32).reshape(-1, 4), z["d0_poses"]
    # a pose far from the cloud: an empty slice
    far = poses[:1].copy()
    far[0, :2] += 5.0e4
    poses = np.concatenate([poses, far])
    points, offsets, _ = D.slice_cloud(cloud, poses)
    off = offsets.cpu().numpy()
    assert points.dtype == torch.float64 and off[-1] == off[-2] and (np.diff(off) > 0).sum() >= 2
    extent = (-35.0, 35.0, -27.0, 27.0)
    maps = B.bev_maps(points, offsets, extent, 0.05)
    assert maps.shape[0] == len(poses) and maps.dtype == torch.float32
    for s in range(len(poses)):
        if off[s + 1] > off[s]:
            one, _ = B.bev_map(points[off[s]:off[s + 1]], 0.05, extent=extent)
            want, _ = R.max_per_pixel(points[off[s]:off[s + 1]].cpu().numpy(), 0.05, None, extent)
            assert torch.equal(maps[s], one) and np.array_equal(one.cpu().numpy(), want)
            assert (one != 0).any()
        else:
            assert not maps[s].any()
    assert torch.equal(maps, B.bev_maps(points, offsets, extent, 0.05))


def test_tone_map_matches_numpy(golden_dir):
    B = _bev()
    z = R.load_g13(golden_dir)
    exact = interpolated = 0
    for k, name, *_ in _clouds(z):
        image = z[f"c{k}_image"]
        norm, p = B.tone_map(torch.from_numpy(image).cuda())
        want_p = z[f"c{k}_p"]
        assert isinstance(p, np.float32)
        ps, st = B.percentile_positive(torch.from_numpy(image).cuda())
        srt = np.sort(image[image > 0])
        m = len(srt)
        vi = np.float32(m - 1) * (np.float32(90) / np.float32(100))           # numpy's index, in the image's dtype
        lo = int(np.floor(vi))
        hi = min(lo + 1, m - 1)
        assert st[0, 0] == m and st[0, 1] == srt[lo] and st[0, 2] == srt[hi], name     # the order statistics are exact
        if st[0, 3] == 0 or srt[lo] == srt[hi]:
            assert p == want_p, name
            exact += 1
        else:
            assert abs(float(p) - float(want_p)) <= float(np.spacing(want_p)), name
            interpolated += 1
        assert np.allclose(norm.cpu().numpy(), z[f"c{k}_norm"], rtol=1e-6, atol=0.0), name
    assert exact and interpolated
    # an image at size with many ties and a non-trivial weight
    rng = np.random.default_rng(8)
    big = np.where(rng.uniform(size=(700, 900)) < 0.4, rng.integers(1, 3000, (700, 900)), 0).astype(np.float32)
    norm, p = B.tone_map(big)
    want_p = np.percentile(big[big > 0], 90)
    assert abs(float(p) - float(want_p)) <= float(np.spacing(want_p))
    assert np.allclose(norm.cpu().numpy(), np.power(np.clip(big / want_p, 0, 1), 0.6), rtol=1e-6, atol=0.0)
    for q in (0.0, 37.5, 100.0):
        ps, _ = B.percentile_positive(big, q)
        w = np.percentile(big[big > 0], q)
        assert abs(float(ps[0]) - float(w)) <= float(np.spacing(w))
    zero = torch.zeros((12, 9), device="cuda")
    norm, p = B.tone_map(zero)
    assert p is None and torch.equal(norm, zero)
    neg = -torch.ones((5, 5), device="cuda")
    norm, p = B.tone_map(neg)
    assert p is None and torch.equal(norm, neg)
    # a stack is tone-mapped slice by slice
    stack = torch.stack([torch.from_numpy(big).cuda(), torch.zeros((700, 900), device="cuda"), torch.from_numpy(big).cuda() * 2])
    norms, ps = B.tone_map(stack)
    assert ps[1] is None and not norms[1].any()
    for s in (0, 2):
        one, p1 = B.tone_map(stack[s])
        assert ps[s] == p1 and torch.equal(norms[s], one)


def test_colorize_equals_matplotlib(golden_dir):
    B = _bev()
    z = R.load_g13(golden_dir)
    for k, name, *_ in _clouds(z):
        image = torch.from_numpy(z[f"c{k}_image"]).cuda()
        norm, _ = B.tone_map(image)
        rgba = B.colorize(norm, image)
        assert rgba.dtype == torch.uint8 and np.array_equal(rgba.cpu().numpy(), z[f"c{k}_rgba"]), name
    x = torch.linspace(0, 1, 4097, device="cuda").reshape(17, 241)
    g = B.colorize(x, torch.ones_like(x), "gray").cpu().numpy()
    idx = np.minimum((x.cpu().numpy() * 256).astype(np.int64), 255)
    assert np.array_equal(g[..., 0], idx) and np.array_equal(g[..., 1], idx) and np.all(g[..., 3] == 255)
    assert g[-1, -1, 0] == 255
    black = B.colorize(x, torch.zeros_like(x)).cpu().numpy()
    assert np.all(black[..., :3] == 0) and np.all(black[..., 3] == 255)


def _canvas(rng, s, h, w):
    c = rng.integers(0, 256, (s, h, w, 4)).astype(np.uint8)
    c[..., 3] = 255
    return c


def _check_draw(got, canvas, window, lines, styles, res):
    want, touched = O.draw(canvas, window, lines, styles, res)
    assert np.abs(got.astype(np.int64) - want.astype(np.int64)).max() <= 1
    assert np.array_equal(got[~touched], canvas[~touched])
    assert np.array_equal(got[..., 3], canvas[..., 3])
    return touched


def test_draw_lines_matches_oracle():
    B = _bev()
    rng = np.random.default_rng(5)
    res = 0.05
    h, w = 150, 210
    window = [-2.0, -2.0 + w * res, 10.0, 10.0 + h * res]      # y_lo, y_hi, x_lo, x_hi
    x_of = lambda v: window[3] - v * res                        # pixel row / column -> metres
    y_of = lambda u: window[0] + u * res
    line = lambda uv: np.array([[x_of(v), y_of(u), 0.0] for u, v in uv])
    t = np.arange(201)
    zig = [(20 + 0.8 * k, 30 + 25 * (k % 2) + 0.1 * k) for k in t]
    zig[-1] = zig[0]                                            # closed, 200 segments
    cases = {
        "horizontal": ([line([(10.3, 40.0), (190.7, 40.0)])], [B.STYLE_GT]),
        "vertical": ([line([(100.5, 5.2), (100.5, 140.9)])], [B.STYLE_REFINED]),
        "diagonal": ([line([(5.0, 5.0), (200.0, 140.0)])], [dict(B.STYLE_GT, alpha=1.0)]),
        "zigzag": ([line(zig)], [B.STYLE_REFINED]),
        "dashed": ([line([(10.0, 20.0), (27.0, 20.0), (120.0, 90.0), (200.0, 95.0)])], [dict(B.STYLE_NOISY, dash=(11.0, 6.0))]),
        "partly_outside": ([line([(-80.0, 60.0), (100.0, 75.0), (300.0, -40.0)])], [B.STYLE_NOISY]),
        "wholly_outside": ([line([(-80.0, -60.0), (-10.0, -5.0)]), line([(400.0, 10.0), (500.0, 900.0)])], [B.STYLE_GT, B.STYLE_GT]),
        "three_in_order": ([line([(10.0, 70.0), (200.0, 80.0)]), line([(10.0, 80.0), (200.0, 70.0)]), line([(100.0, 10.0), (110.0, 140.0)])],
                           [B.STYLE_GT, B.STYLE_NOISY, B.STYLE_REFINED]),
        "degenerate": ([line([(50.0, 50.0), (50.0, 50.0), (60.0, 50.0)]), line([(5.0, 5.0)])], [B.STYLE_GT, B.STYLE_GT]),
    }
    for name, (lines, styles) in cases.items():
        canvas = _canvas(rng, 1, h, w)[0]
        dev = torch.from_numpy(canvas.copy()).cuda()
        out = B.draw_lines(dev, window, lines, [0] * len(lines), styles, res)
        assert out is dev
        got = dev.cpu().numpy()
        touched = _check_draw(got, canvas, window, lines, styles, res)
        assert touched.any() == (name != "wholly_outside"), name
        again = torch.from_numpy(canvas.copy()).cuda()
        B.draw_lines(again, window, lines, [0] * len(lines), styles, res)
        assert torch.equal(dev, again), name
    # zero lines: nothing changes
    canvas = _canvas(rng, 2, 40, 50)
    dev = torch.from_numpy(canvas.copy()).cuda()
    B.draw_lines(dev, [[0, 2.5, 0, 2], [0, 2.5, 0, 2]], [], [], [], res)
    assert np.array_equal(dev.cpu().numpy(), canvas)
    with pytest.raises(ValueError):
        B.draw_lines(dev, [[0, 2.5, 0, 2], [0, 2.5, 0, 2]], [line([(1, 1), (2, 2)])], [2], [B.STYLE_GT], res)


def test_draw_lines_batches_views_of_different_sizes():
    B = _bev()
    rng = np.random.default_rng(6)
    res = 0.1
    image = torch.from_numpy(_canvas(rng, 1, 300, 400)[0]).cuda()
    extent = [-20.0, 20.0, -15.0, 15.0]
    windows = [[-10.0, 3.3, -5.0, 4.1], [2.0, 19.0, -14.0, 14.0], [-1.0, 1.0, -1.0, 1.0]]
    views = B.crop_views(image, extent, windows, res)
    assert len(views) == 3 and len({tuple(s) for s in views.shapes}) == 3
    before = [views[k].cpu().numpy().copy() for k in range(3)]
    lines, line_view, styles = [], [], []
    for k, wdw in enumerate(views.windows):
        for j, st in enumerate((B.STYLE_GT, B.STYLE_NOISY, B.STYLE_REFINED)):
            n = 12
            x = np.linspace(wdw[2] - 1.0, wdw[3] + 1.0, n)
            y = np.linspace(wdw[0], wdw[1], n) + 0.3 * j + rng.normal(0, 0.2, n)
            lines.append(np.column_stack([x, y, np.zeros(n)])); line_view.append(k); styles.append(st)
    order = rng.permutation(len(lines))                         # lines of different views interleaved
    lines, line_view, styles = [lines[i] for i in order], [line_view[i] for i in order], [styles[i] for i in order]
    B.draw_lines(views, None, lines, line_view, styles)
    for k in range(3):
        mine = [i for i, v in enumerate(line_view) if v == k]
        _check_draw(views[k].cpu().numpy(), before[k], views.windows[k], [lines[i] for i in mine], [styles[i] for i in mine], res)
    # the same through an (S, H, W, 4) tensor
    stack = torch.from_numpy(_canvas(rng, 2, 64, 80)).cuda()
    orig = stack.cpu().numpy().copy()
    wins = [[0.0, 8.0, 0.0, 6.4], [10.0, 18.0, -3.0, 3.4]]
    ls = [np.array([[1.0, 1.0], [5.0, 7.0]]), np.array([[-2.0, 11.0], [3.0, 17.5]])]
    B.draw_lines(stack, wins, ls, [0, 1], [B.STYLE_GT, B.STYLE_REFINED], res)
    for k in range(2):
        _check_draw(stack[k].cpu().numpy(), orig[k], wins[k], [ls[k]], [[B.STYLE_GT, B.STYLE_REFINED][k]], res)


def test_crop_views_equals_numpy_indexing():
    B = _bev()
    rng = np.random.default_rng(7)
    res = 0.05
    img = _canvas(rng, 1, 240, 320)[0]
    y_min, x_max = -8.0, 6.0
    extent = [y_min, y_min + 320 * res, x_max - 240 * res, x_max]
    windows = np.array([[-6.0, -1.0, 0.0, 4.0],                 # inside
                        [-9.03, -5.5, 3.0, 7.21],               # across the top-left border
                        [6.0, 9.5, -7.5, -4.0],                 # across the bottom-right border
                        [30.0, 32.0, 30.0, 31.0],               # outside
                        [-8.0, 8.0, -6.0, 6.0],                 # the whole image
                        [0.0, 0.01, 0.0, 0.01]])                # smaller than a pixel: 1 x 1
    views = B.crop_views(torch.from_numpy(img).cuda(), extent, windows, res)
    padded = np.zeros((240 + 2000, 320 + 2000, 4), dtype=np.uint8)
    padded[..., 3] = 255
    padded[1000:1240, 1000:1320] = img
    for k, wdw in enumerate(windows):
        u0, v0 = int(np.floor((wdw[0] - y_min) / res)), int(np.floor((x_max - wdw[3]) / res))
        w = max(int(np.floor((wdw[1] - wdw[0]) / res + 0.5)), 1)
        h = max(int(np.floor((wdw[3] - wdw[2]) / res + 0.5)), 1)
        assert tuple(views.shapes[k]) == (h, w)
        want = padded[1000 + v0:1000 + v0 + h, 1000 + u0:1000 + u0 + w]
        assert np.array_equal(views[k].cpu().numpy(), want), k
        assert np.abs(views.windows[k] - wdw).max() < 1.5 * res + 1e-9 or k == 5
    assert np.array_equal(views[4].cpu().numpy(), img)
    assert not views[3].cpu().numpy()[..., :3].any()
    empty = B.crop_views(torch.from_numpy(img).cuda(), extent, np.zeros((0, 4)), res)
    assert len(empty) == 0 and empty.data.shape == (0, 4)


def test_chamfer_xy_equals_reference(golden_dir):
    B = _bev()
    z = R.load_g13(golden_dir)
    gts = np.split(z["cm_gt"], np.cumsum(z["cm_gt_len"])[:-1])
    preds = np.split(z["cm_pred"], np.cumsum(z["cm_pred_len"])[:-1])
    got = B.chamfer_xy(gts, preds)
    assert np.all(np.abs(got - z["cm_val"]) <= 1e-12 * np.abs(z["cm_val"]))
    mixed = B.chamfer_xy([None, gts[0], np.zeros((0, 3))], [preds[0], preds[0], preds[1]])
    assert mixed[0] == -1.0 and mixed[2] == -1.0 and abs(mixed[1] - z["cm_val"][0]) <= 1e-12 * z["cm_val"][0]


def _scene(seed=9):
    rng = np.random.default_rng(seed)
    items = []
    for i in range(5):
        n = int(rng.integers(5, 20))
        x = np.sort(rng.uniform(-18, 18, n))
        gt = np.stack([x, 3.0 * i - 6 + 0.2 * np.sin(x / 5.0), np.zeros(n)], 1)
        cx = np.linspace(-15, 15, 9)
        cand = np.stack([cx, 3.0 * i - 6 + 0.2 * np.sin(cx / 5.0) + rng.uniform(-0.4, 0.4), rng.normal(0, 0.02, 9)], 1)
        items.append({"position": gt, "noisy_candidates": [cand, cand + 0.1], "context_lines": []})
    items[1]["position"] = None                                  # no GT: error -1
    items[2]["noisy_candidates"] = []                            # GT only: no refinement
    items.append({"position": None, "noisy_candidates": [], "context_lines": []})       # skipped
    items[4]["noisy_candidates"] = [items[4]["noisy_candidates"][0][:1]]                 # a 1-vertex candidate
    xyz = np.stack([rng.uniform(-20, 20, 40000), rng.uniform(-9, 9, 40000), rng.normal(0, 0.05, 40000)], 1)
    cloud = np.column_stack([xyz, rng.integers(1, 4000, 40000)]).astype(np.float32)
    return items, cloud


def test_render_scene_is_the_pipeline_by_hand(tmp_path):
    B = _bev()
    from oracle import procedural as P
    from pointnet_refine_amd.context import resample_polyline
    from pointnet_refine_amd.io import refine_scene
    from pointnet_refine_amd.model import LineRefineNet
    items, cloud = _scene()
    m = LineRefineNet()
    m.load_state_dict(P.linerefine_state_dict(0))
    m = m.cuda()
    res = B.render_scene(m, cloud, items, out_dir=str(tmp_path), name="s7", num_context_points=256)
    assert res["items"] == [0, 1, 2, 3, 4]
    # by hand
    image, extent = B.bev_map(cloud)
    norm, p = B.tone_map(image)
    rgba = B.colorize(norm, image)
    windows, kept = B.item_windows(items)
    views = B.crop_views(rgba, extent, windows)
    rows = [0, 1, 3]
    again, again_noisy = refine_scene(m, cloud, [items[i]["noisy_candidates"][0] for i in rows], 32, 256, 0.5)
    refined, noisy = [res["refined"][i] for i in rows], [res["noisy"][i] for i in rows]
    assert np.abs(np.array(refined) - again).max() < 1e-4 and np.abs(np.array(noisy) - again_noisy).max() < 1e-9
    assert [k for k, r in enumerate(res["refined"]) if r is not None] == rows
    lines, lv, st = [], [], []
    for k, i in enumerate(kept):
        gt = items[i]["position"]
        if gt is not None and len(gt) > 1:
            lines.append(gt); lv.append(k); st.append(B.STYLE_GT)
        if i in rows:
            lines += [items[i]["noisy_candidates"][0], refined[rows.index(i)]]
            lv += [k, k]; st += [B.STYLE_NOISY, B.STYLE_REFINED]
    B.draw_lines(views, None, lines, lv, st)
    assert torch.equal(res["image"], image) and res["p"] == p and np.array_equal(res["windows"], views.windows)
    assert torch.equal(res["views"].data, views.data)
    assert (views.data != B.crop_views(rgba, extent, windows).data).any()
    # errors: chamfer_xy against the resampled GT
    gt_res = [resample_polyline(items[i]["position"], 32) if items[i]["position"] is not None else None for i in rows]
    e_noisy, e_ref = B.chamfer_xy(gt_res, list(noisy)), B.chamfer_xy(gt_res, list(refined))
    assert np.array_equal(res["err_noisy"][rows], e_noisy) and np.array_equal(res["err_refined"][rows], e_ref)
    assert res["err_noisy"][1] == -1.0 and np.isnan(res["err_noisy"][2]) and np.isnan(res["err_refined"][4])
    # files
    doc = json.load(open(tmp_path / "s7.json"))
    assert [e["item"] for e in doc["items"]] == kept
    for k, e in enumerate(doc["items"]):
        png = R.read_png(str(tmp_path / f"s7_item_{e['item']}.png"))
        assert np.array_equal(png, res["views"][k].cpu().numpy())
        assert e["window"] == [float(v) for v in views.windows[k]]
        if e["item"] in rows:
            r = rows.index(e["item"])
            assert e["err_noisy"] == e_noisy[r] and e["err_refined"] == e_ref[r]
            assert e["noisy_label"] == f"Noisy (E={e_noisy[r]:.2f}m)" and e["refined_label"] == f"Refined (E={e_ref[r]:.2f}m)"
        else:
            assert "err_noisy" not in e
    assert sorted(os.listdir(tmp_path)) == sorted([f"s7_item_{i}.png" for i in kept] + ["s7.json"])


def test_render_sample_draws_the_three_lines():
    B = _bev()
    from pointnet_refine_amd.synth import synthetic_batch
    ctx, noisy, target = synthetic_batch(2, 512, torch.device("cuda"), seed=3)
    pic = B.render_sample(ctx, noisy, 0.5 * target, target)
    assert pic.dtype == torch.uint8 and pic.dim() == 3 and pic.shape[2] == 4
    img = pic.cpu().numpy()
    flat = img.reshape(-1, 4)
    assert (flat[:, 3] == 255).all()
    for colour in ((255, 0, 0), (0, 255, 0), (0, 255, 255)):
        assert (np.abs(flat[:, :3].astype(int) - np.array(colour)).max(1) <= 1).any(), colour
    assert torch.equal(pic, B.render_sample(ctx, noisy, 0.5 * target, target))
