"""3-D views on the GPU (csrc/prh_view.hpp through pointnet_refine_amd.view3d) against the numpy
restatement of the rule in _view3d_oracle.py: depth buffers word for word, RGBA and depth bit for
bit, no pixel left out, no tolerance.  Images are 33 x 47: no multiple of a wave or a tile."""
import functools
import json
import os

import numpy as np
import pytest
import torch

import _view3d_oracle as O
import make_golden_g14_view3d as M
import test_bev_cpu as R

pytestmark = pytest.mark.gpu

H, W = M.H, M.W


def _view():
    from pointnet_refine_amd import view3d
    return view3d


def words(z):
    return z.cpu().numpy().view(np.uint64)


@functools.lru_cache(maxsize=None)
def _cloud(dtype_name):
    pts, cams = M.cloud(np.dtype(dtype_name).type)
    pts.setflags(write=False); cams.setflags(write=False)
    return pts, cams


@functools.lru_cache(maxsize=None)
def _oracle_splat(dtype_name, n, v, k):
    pts, cams = _cloud(dtype_name)
    z = O.new_zbuffer(v, H, W)
    stats = O.splat(z, pts[:n], cams[:v], k, M.CMIN, M.CMAX)
    z.setflags(write=False)
    return z, stats


@pytest.mark.parametrize("k", [1, 2, 3])
@pytest.mark.parametrize("v", [1, 3])
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("n", [0, 1, 257, 5000])
def test_splat_equals_oracle_word_for_word(n, dtype, v, k):
    V = _view()
    name = np.dtype(dtype).name
    pts, cams = _cloud(name)
    want, stats = _oracle_splat(name, n, v, k)
    if n == 5000:                        # the cloud exercises what it is meant to (on the oracle's own output)
        for view, (landed, hits, tied) in enumerate(stats):
            assert landed >= n // 2, (view, landed)
            assert (hits >= 2).sum() >= 100, view
            assert tied >= 1, view
            assert hits[0].sum() and hits[-1].sum() and hits[:, 0].sum() and hits[:, -1].sum(), view
        xr, yu, d = O.view_space(pts[:2, :3].astype(np.float64), cams[0])
        assert d[0] == cams[0, 13] and d[1] < cams[0, 13]                      # exactly at near / just nearer
        inten = pts[:, 3]
        assert (inten < M.CMIN).sum() > 100 and (inten > M.CMAX).sum() > 100
        behind = sum(int((O.view_space(pts[:, :3].astype(np.float64), c)[2] < c[13]).sum()) for c in cams[:v])
        assert behind >= 10
    if n == 1:                           # the point exactly at d == near is drawn
        assert (want[0] != O.EMPTY).sum() >= 1
    z = V.new_zbuffer(v, H, W)
    assert (words(z) == O.EMPTY).all()
    out = V.splat_points(z, pts[:n], cams[:v], k, M.CMIN, M.CMAX)
    assert out is z
    assert np.array_equal(words(z), want)


def test_splat_equals_the_fixture(golden_dir):
    V = _view()
    g = np.load(os.path.join(golden_dir, "g14_view3d.npz"))
    z = V.new_zbuffer(3, H, W)
    V.splat_points(z, g["points"], g["cameras"], 2, M.CMIN, M.CMAX)
    assert np.array_equal(words(z), g["splat_words"])
    lines, styles, _ = M.lines_scene(g["cameras"])
    V.draw_lines3d(z, lines, styles, g["cameras"])
    assert np.array_equal(words(z), g["words"])
    rgba, depth = V.resolve(z, M.table(), styles, (7, 8, 9))
    assert np.array_equal(rgba.cpu().numpy(), g["rgba"])
    assert np.array_equal(depth.cpu().numpy().view(np.uint32), g["depth"].view(np.uint32))


@pytest.mark.parametrize("k", [1, 9])
def test_splat_every_size_up_to_nine(k):
    V = _view()
    pts, cams = _cloud("float32")
    want, _ = _oracle_splat("float32", 600, 3, k)
    z = V.splat_points(V.new_zbuffer(3, H, W), pts[:600], cams, k, M.CMIN, M.CMAX)
    assert np.array_equal(words(z), want)
    with pytest.raises(ValueError):
        V.splat_points(z, pts[:10], cams, 10, M.CMIN, M.CMAX)
    with pytest.raises(ValueError):
        V.splat_points(z, pts[:10], cams, 0, M.CMIN, M.CMAX)


def test_splat_does_not_depend_on_order_and_csr_equals_slices():
    V = _view()
    pts, cams = _cloud("float32")
    want, _ = _oracle_splat("float32", 5000, 3, 2)
    rng = np.random.default_rng(3)
    for _ in range(3):
        perm = rng.permutation(len(pts))
        z = V.splat_points(V.new_zbuffer(3, H, W), torch.from_numpy(pts[perm]).cuda(), cams, 2, M.CMIN, M.CMAX)
        assert np.array_equal(words(z), want)
    # CSR: five slices (one empty), each into its own views
    offsets = np.array([0, 700, 700, 2100, 3333, 5000])
    slice_view = [[0], [1], [1, 2], [], [0, 2]]
    z = V.splat_points(V.new_zbuffer(3, H, W), pts, cams, 2, M.CMIN, M.CMAX, offsets=offsets, slice_view=slice_view)
    by_hand = V.new_zbuffer(3, H, W)
    for s, views in enumerate(slice_view):
        for view in views:
            V.splat_points(by_hand[view:view + 1], pts[offsets[s]:offsets[s + 1]], cams[view:view + 1], 2, M.CMIN, M.CMAX)
    assert torch.equal(z, by_hand)
    mask = np.zeros((5, 3), dtype=np.uint8)
    for s, views in enumerate(slice_view):
        mask[s, views] = 1
    want = O.new_zbuffer(3, H, W)
    O.splat(want, pts, cams, 2, M.CMIN, M.CMAX, offsets, mask)
    assert np.array_equal(words(z), want)
    one_each = V.splat_points(V.new_zbuffer(3, H, W), pts, cams, 2, M.CMIN, M.CMAX, offsets=offsets,
                              slice_view=np.array([0, 1, 2, -1, 1]))
    want = O.new_zbuffer(3, H, W)
    O.splat(want, pts, cams, 2, M.CMIN, M.CMAX, offsets, np.array([[1, 0, 0], [0, 1, 0], [0, 0, 1], [0, 0, 0], [0, 1, 0]]))
    assert np.array_equal(words(one_each), want)


def test_top_down_lattice_occupies_the_pixels_bev_map_occupies():
    """The camera convention, independently of the oracle.  Points sit at pixel centres of a 1 / 8 m
    lattice.  bev_map over extent (y_min, y_max, x_min, x_max) puts (x, y) at column (y - y_min) / res
    and row (x_max - x) / res.  A top-down orthographic camera (elev 90) at azim 180 has right = -y
    and up = +x, so its column grows with -y and its row with -x, like bev_map's row; the mapping is
    therefore view[row, col] <-> bev[row, W - 1 - col]."""
    V = _view()
    from pointnet_refine_amd import bev
    res, h, w = 0.125, 24, 40
    rng = np.random.default_rng(5)
    rows, cols = rng.integers(0, h, 300), rng.integers(0, w, 300)
    x_max, y_min = 2.0, -3.0
    pts = np.column_stack([x_max - (rows + 0.5) * res, y_min + (cols + 0.5) * res, rng.uniform(-0.5, 0.5, 300),
                           rng.uniform(1, 50, 300)]).astype(np.float32)
    image, _ = bev.bev_map(pts, res, extent=(y_min, y_min + w * res, x_max - h * res, x_max))
    occupied = image.cpu().numpy() > 0
    assert occupied.shape == (h, w) and occupied.sum() == len(set(zip(rows, cols)))
    centre = (x_max - h * res / 2, y_min + w * res / 2, 0.0)
    cam = V.orbit_camera(centre, 90.0, 180.0, 10.0, ortho_scale=1.0 / res, near=0.5, height=h, width=w)
    z = V.splat_points(V.new_zbuffer(1, h, w), pts, cam[None], 1, 0.0, 50.0)
    filled = words(z)[0] != O.EMPTY
    assert np.array_equal(filled, occupied[:, ::-1])
    # and the depth is the height below the eye
    _, depth = V.resolve(z, V.gray_table())
    d = depth.cpu().numpy()[0]
    assert np.isposinf(d[~filled]).all() and (np.abs(d[filled] - 10.0) <= 0.5 + 1e-6).all()


def _lines_case(with_cloud):
    V = _view()
    lines, styles, cams = M.lines_scene()
    pts, ccams = _cloud("float32")
    cams[0, 13] = ccams[0, 13]
    want = O.new_zbuffer(3, H, W)
    z = V.new_zbuffer(3, H, W)
    if with_cloud:
        O.splat(want, pts[:1500], cams, 2, M.CMIN, M.CMAX)
        V.splat_points(z, pts[:1500], cams, 2, M.CMIN, M.CMAX)
    segs, ids = O.segments(lines, cams, H, W)
    O.draw(want, segs, ids, styles, cams)
    V.draw_lines3d(z, lines, styles, cams)
    return V, z, want, lines, styles, cams


@pytest.mark.parametrize("with_cloud", [False, True])
def test_lines_equal_oracle_word_for_word(with_cloud):
    V, z, want, lines, styles, cams = _lines_case(with_cloud)
    got = words(z)
    assert np.array_equal(got, want)
    if with_cloud:
        return
    pay = (want & np.uint64(0xFFFFFFFF)).astype(np.int64)
    drawn = want != O.EMPTY
    for view in range(3):                               # perspective (0, 2) and orthographic (1) views
        seen = set(pay[view][drawn[view]].tolist())
        assert {0, 1, 2, 3, 4, 7, 8, 9} <= seen, (view, seen)
    assert 5 in set(pay[0][drawn[0]].tolist()) and 6 not in set(pay[0][drawn[0]].tolist())
    # the dashed line has gaps, the markers-only line is three separate discs
    solid = [dict(s, dash=None) for s in styles]
    full = O.new_zbuffer(3, H, W)
    segs, ids = O.segments(lines, cams, H, W)
    O.draw(full, segs, ids, solid, cams)
    assert ((full & np.uint64(0xFFFFFFFF)) == 1).sum() > (pay == 1)[drawn].sum() > 0
    # two lines crossing at equal depth under the camera that looks straight down: the lower index wins
    only = O.new_zbuffer(1, H, W)
    s9, i9 = O.segments([lines[9]], cams[2:3], H, W)
    O.draw(only, s9, i9, [styles[9]], cams[2:3])
    s8, i8 = O.segments([lines[8]], cams[2:3], H, W)
    eight = O.new_zbuffer(1, H, W)
    O.draw(eight, s8, i8, [styles[8]], cams[2:3])
    both = (only[0] != O.EMPTY) & (eight[0] != O.EMPTY)
    assert both.sum() >= 1 and ((only[0] >> np.uint64(32)) == (eight[0] >> np.uint64(32)))[both].all()
    assert (pay[2][both] != 9).all() and (pay[2][both] == 8).any()


def test_line_behind_a_wall_is_hidden_and_a_bias_brings_it_forward():
    V = _view()
    cam = V.orbit_camera((0.0, 0.0, 0.0), 90.0, 0.0, 10.0, ortho_scale=4.0, near=0.5, height=H, width=W)[None]
    gx, gy = np.meshgrid(np.arange(-6, 6, 0.2), np.arange(-8, 8, 0.2))
    wall = np.column_stack([gx.ravel(), gy.ravel(), np.full(gx.size, 1.0), np.full(gx.size, 20.0)]).astype(np.float32)
    line = [np.array([[-3.0, -4.0, 0.5], [3.0, 4.0, 0.5]])]
    for bias, visible in ((0.0, False), (0.75, True)):
        style = [{"color": (255, 0, 0), "width": 3.0, "marker": 0.0, "dash": None, "bias": bias}]
        want = O.new_zbuffer(1, H, W)
        O.splat(want, wall, cam, 3, M.CMIN, M.CMAX)
        assert (want != O.EMPTY).all()
        segs, ids = O.segments(line, cam, H, W)
        O.draw(want, segs, ids, style, cam)
        z = V.splat_points(V.new_zbuffer(1, H, W), wall, cam, 3, M.CMIN, M.CMAX)
        V.draw_lines3d(z, line, style, cam)
        assert np.array_equal(words(z), want)
        n_line = int(((want & np.uint64(0x01000000)) == 0).sum())
        assert (n_line > 30) if visible else (n_line == 0)


def test_resolve_equals_oracle():
    V, z, want, lines, styles, cams = _lines_case(True)
    for table, background in ((M.table(), (7, 8, 9)), (V.viridis_table(), (255, 255, 255))):
        rgba, depth = V.resolve(z, table, styles, background)
        want_rgba, want_depth = O.resolve(want, table, styles, background)
        assert rgba.dtype == torch.uint8 and tuple(rgba.shape) == (3, H, W, 4) and depth.dtype == torch.float32
        assert np.array_equal(rgba.cpu().numpy(), want_rgba)
        assert np.array_equal(depth.cpu().numpy().view(np.uint32), want_depth.view(np.uint32))
    empty = want == O.EMPTY
    assert empty.sum() > 50 and np.isposinf(want_depth[empty]).all() and (want_rgba[empty] == (255, 255, 255, 255)).all()
    assert torch.equal(z, torch.from_numpy(want.view(np.int64)).cuda())          # resolve leaves the buffer alone


def test_bad_input_raises_and_reads_nothing_out_of_bounds():
    V = _view()
    pts, cams = _cloud("float32")
    for column in range(4):
        for value in (np.nan, np.inf):
            bad = pts[:513].copy()
            bad[512, column] = value                     # the last point of the last block
            with pytest.raises(ValueError):
                V.splat_points(V.new_zbuffer(3, H, W), bad, cams, 2, M.CMIN, M.CMAX)
            with pytest.raises(ValueError):
                V.view_bounds(bad)
    bad = pts[:300].astype(np.float64)
    bad[0, 2] = -np.inf
    with pytest.raises(ValueError):
        V.splat_points(V.new_zbuffer(1, H, W), bad, cams[:1], 1, M.CMIN, M.CMAX)
    lo, hi = V.view_bounds(pts)
    assert np.array_equal(lo, pts[:, :3].min(0).astype(np.float64)) and np.array_equal(hi, pts[:, :3].max(0).astype(np.float64))
    lo, hi = V.view_bounds(pts[:1].astype(np.float64))
    assert np.array_equal(lo, pts[0, :3]) and np.array_equal(hi, pts[0, :3])
    with pytest.raises(ValueError):
        V.splat_points(V.new_zbuffer(2, H, W), pts, cams, 1, M.CMIN, M.CMAX)      # three cameras, two views
    with pytest.raises(ValueError):
        V.splat_points(V.new_zbuffer(3, H, W), pts, cams, 1, 5.0, 5.0)


def _scene(seed=11):
    rng = np.random.default_rng(seed)
    items = []
    for i in range(3):
        x = np.linspace(-8, 8, 7)
        gt = np.stack([x, 3.0 * i - 3 + 0.2 * np.sin(x / 3.0), np.zeros(7)], 1)
        cx = np.linspace(-7, 7, 6)
        cand = np.stack([cx, 3.0 * i - 3 + 0.2 * np.sin(cx / 3.0) + rng.uniform(-0.3, 0.3), rng.normal(0, 0.02, 6)], 1)
        items.append({"position": gt, "noisy_candidates": [cand], "context_lines": []})
    items[0]["context_lines"] = [np.stack([x, np.full(7, 5.0), np.zeros(7)], 1)]
    items[2]["position"] = None                                     # no GT: no metric string
    xyz = np.stack([rng.uniform(-10, 10, 2000), rng.uniform(-6, 6, 2000), rng.normal(0, 0.03, 2000)], 1)
    cloud = np.column_stack([xyz, rng.integers(1, 60, 2000)]).astype(np.float32)
    return items, cloud


def test_render_scene3d_is_the_pipeline_by_hand(tmp_path):
    V = _view()
    from oracle import procedural as P
    from pointnet_refine_amd.metrics import evaluate_scene
    from pointnet_refine_amd.model import LineRefineNet
    items, cloud = _scene()
    m = LineRefineNet()
    m.load_state_dict(P.linerefine_state_dict(0))
    m = m.cuda()
    h, w = 90, 130
    res = V.render_scene3d(m, cloud, items, out_dir=str(tmp_path), name="s3", closeups=True, num_context_points=256,
                           height=h, width=w)
    assert res["view_items"] == [-1, 0, 1, 2] and tuple(res["rgba"].shape) == (4, h, w, 4)
    # by hand, from the low-level calls
    ev = evaluate_scene(m, cloud, items, 32, 256, 0.3)
    assert np.abs(ev["refined"] - res["eval"]["refined"]).max() < 1e-4
    lines = [items[0]["context_lines"][0], items[0]["position"], res["eval"]["noisy"][0], res["eval"]["refined"][0],
             items[1]["position"], res["eval"]["noisy"][1], res["eval"]["refined"][1], res["eval"]["noisy"][2],
             res["eval"]["refined"][2]]
    styles = [V.STYLE_CONTEXT_GT, V.STYLE_GT, V.STYLE_NOISY, V.STYLE_REFINED, V.STYLE_GT, V.STYLE_NOISY, V.STYLE_REFINED,
              V.STYLE_NOISY, V.STYLE_REFINED]
    assert len(res["lines"]) == 9 and all(np.array_equal(a, b) for a, b in zip(res["lines"], lines)) and res["styles"] == styles
    lo, hi = V.view_bounds(cloud)
    cams = [V.fit_camera((lo, hi), 35.0, 180.0, height=h, width=w, target=(0, 0, 0))]
    for group in (lines[1:4], lines[4:7], lines[7:9]):
        v = np.concatenate(group)
        cams.append(V.fit_camera((v.min(0) - 5.0, v.max(0) + 5.0), 35.0, 180.0, height=h, width=w))
    cams = np.stack(cams)
    assert np.array_equal(res["cameras"], cams)
    z = V.new_zbuffer(4, h, w)
    V.splat_points(z, cloud, cams, 2, 1.0, 40.0)
    only_points = z.clone()
    V.draw_lines3d(z, lines, styles, cams)
    rgba, depth = V.resolve(z, V.jet_table(), styles)
    assert torch.equal(res["zbuf"], z) and torch.equal(res["rgba"], rgba) and torch.equal(res["depth"], depth)
    assert (z != only_points).any()
    pay = words(z) & np.uint64(0xFFFFFFFF)
    for view in range(4):
        assert ((pay[view] < 0x01000000) & (words(z)[view] != O.EMPTY)).sum() > 20, view
    # labels: the reference's legend names, metric strings where there is a GT
    e = res["eval"]
    info = [f"<br>ADE: {e['ade_noisy'][r]:.2f}->{e['ade_refined'][r]:.2f}<br>Lat: {e['lat_noisy'][r]:.2f}->{e['lat_refined'][r]:.2f}"
            for r in range(2)]
    assert e["valid"].tolist() == [True, True, False] and not e["bad_match"].any()
    assert res["labels"] == ["Context GT", "GT Line 0", "Noisy 0" + info[0], "Refined 0", "GT Line 1", "Noisy 1" + info[1],
                             "Refined 1", "Noisy 2", "Refined 2"]
    # files
    doc = json.load(open(tmp_path / "s3.json"))
    assert [v["item"] for v in doc["views"]] == [-1, 0, 1, 2]
    assert [l["label"] for l in doc["lines"]] == res["labels"] and len(doc["lines"]) == len(lines)
    assert [l["color"] for l in doc["lines"]] == [list(s["color"]) for s in styles]
    host = res["rgba"].cpu().numpy()
    for k, view in enumerate(doc["views"]):
        assert view["camera"] == [float(x) for x in cams[k]]
        assert np.array_equal(R.read_png(str(tmp_path / view["file"])), host[k])
    assert sorted(os.listdir(tmp_path)) == sorted([f"s3_view_{k}.png" for k in range(4)] + ["s3.json"])


def _has(rgba, colour):
    flat = rgba.cpu().numpy().reshape(-1, 4)
    return bool((flat[:, :3] == np.array(colour, dtype=np.uint8)).all(1).any()) and bool((flat[:, 3] == 255).all())


def test_render_sample3d_and_render_cloud3d_draw_every_line_colour():
    V = _view()
    from pointnet_refine_amd.synth import synthetic_batch
    ctx, noisy, target = synthetic_batch(2, 512, torch.device("cuda"), seed=3)
    keep = [t.clone() for t in (ctx, noisy, target)]
    out = V.render_sample3d(ctx, noisy, target, height=120, width=160)
    assert tuple(out["rgba"].shape) == (120, 160, 4) and out["cameras"].shape == (1, 16)
    assert _has(out["rgba"], (255, 0, 0)) and _has(out["rgba"], (0, 128, 0)) and _has(out["rgba"], (255, 255, 255))
    assert all(torch.equal(a, b) for a, b in zip(keep, (ctx, noisy, target)))
    again = V.render_sample3d(ctx, noisy, target, height=120, width=160)
    assert torch.equal(out["rgba"], again["rgba"]) and torch.equal(out["zbuf"], again["zbuf"])
    items, cloud = _scene()
    cloud_t = torch.from_numpy(cloud).cuda()
    keep = cloud_t.clone()
    gts = [items[0]["position"], items[1]["position"], items[0]["context_lines"][0]]
    cands = [it["noisy_candidates"][0] + np.array([0.0, 0.7 * k, 0.3]) for k, it in enumerate(items)]
    out = V.render_cloud3d(cloud_t, gts, categories=["lane_line", "curb", "stop_line"], candidates=cands, height=150, width=200)
    assert tuple(out["rgba"].shape) == (150, 200, 4) and len(out["labels"]) == 6
    for colour in ((255, 0, 0), (255, 165, 0), (0, 0, 255), (0, 255, 255), (255, 255, 0), (255, 0, 255)):
        assert _has(out["rgba"], colour), colour
    assert torch.equal(cloud_t, keep)
    table = V.viridis_table()
    flat = out["rgba"].cpu().numpy().reshape(-1, 4)
    assert (flat[:, None, :] == table[None, :, :]).all(2).any(1).sum() > 500          # the cloud shows in viridis


def test_render_drive3d_is_the_merged_cloud_and_every_slice_in_its_own_view(tmp_path):
    V = _view()
    import test_drive_gpu as TD
    from pointnet_refine_amd import drive as D
    drive_dir, out_dir = str(tmp_path / "drive"), str(tmp_path / "out")
    os.makedirs(drive_dir)
    gt, cloud, poses = TD._write_drive(drive_dir)
    cloud[:, 2] = 5.0 + np.random.default_rng(2).normal(0, 0.03, len(cloud))       # a road surface at the lanes' height
    with open(os.path.join(drive_dir, "merged.pcd"), "wb") as f:
        f.write((f"VERSION 0.7\nFIELDS x y z intensity\nSIZE 4 4 4 4\nTYPE F F F F\nCOUNT 1 1 1 1\nWIDTH {len(cloud)}\n"
                 f"HEIGHT 1\nVIEWPOINT 0 0 0 1 0 0 0\nPOINTS {len(cloud)}\nDATA binary\n").encode())
        f.write(cloud.astype("<f4").tobytes())
    h, w = 90, 130
    res = V.render_drive3d(drive_dir, gt, out_dir=out_dir, name="d", max_slices=3, height=h, width=w)
    chosen = D.plan_slices(poses)[:3]
    assert len(chosen) == 3 and res["names"] == [f"{j:06d}" for j in chosen] and tuple(res["rgba"].shape) == (4, h, w, 4)
    # by hand: the slices one call each instead of one CSR call
    cloud32 = np.ascontiguousarray(cloud[:, :4], dtype=np.float32)
    points, offsets, _ = D.slice_cloud(cloud32, np.asarray(poses, dtype=np.float64)[chosen])
    assert torch.equal(points, res["points"]) and torch.equal(offsets, res["offsets"])
    off = offsets.cpu().numpy()
    assert (np.diff(off) > 100).all()
    cams = res["cameras"]
    assert np.array_equal(cams[1], cams[2]) and np.array_equal(cams[0], V.fit_camera(V.view_bounds(cloud32), 35.0, 180.0,
                                                                                     height=h, width=w))
    z = V.new_zbuffer(4, h, w)
    V.splat_points(z[0:1], cloud32, cams[0:1], 2, 0.0, 30.0)
    for s in range(3):
        V.splat_points(z[1 + s:2 + s], points[off[s]:off[s + 1]], cams[1 + s:2 + s], 2, 0.0, 30.0)
    only_points = z.clone()
    V.draw_lines3d(z, res["lines"], res["styles"], cams, res["line_views"])
    assert torch.equal(z, res["zbuf"]) and (z != only_points).any()
    rgba, depth = V.resolve(z, V.viridis_table(), res["styles"])
    assert torch.equal(rgba, res["rgba"]) and torch.equal(depth, res["depth"])
    # three GT lines in the merged view, the clipped ones in their slices only; every view shows points and lines
    assert res["line_views"][:3] == [[0], [0], [0]] and len(res["lines"]) > 3
    assert sorted({v[0] for v in res["line_views"][3:]}) == [1, 2, 3] and len(res["labels"]) == len(res["lines"])
    wd = words(z)
    pay = wd & np.uint64(0xFFFFFFFF)
    for view in range(4):
        drawn = wd[view] != O.EMPTY
        assert (drawn & (pay[view] >= 0x01000000)).sum() > (200 if view else 50), view
        mine = {l for l, v in enumerate(res["line_views"]) if v == [view]}
        shown = set(pay[view][drawn & (pay[view] < 0x01000000)].astype(int).tolist())
        assert shown and shown <= mine, view
    assert not torch.equal(res["rgba"][1], res["rgba"][2])
    # files
    doc = json.load(open(os.path.join(out_dir, "d.json")))
    assert [v["file"] for v in doc["views"]] == ["d_merged.png"] + [f"d_slice_{n}.png" for n in res["names"]]
    assert [l["label"] for l in doc["lines"]] == res["labels"] and [l["views"] for l in doc["lines"]] == res["line_views"]
    host = res["rgba"].cpu().numpy()
    for k, view in enumerate(doc["views"]):
        assert view["camera"] == [float(x) for x in cams[k]]
        assert np.array_equal(R.read_png(os.path.join(out_dir, view["file"])), host[k])
    with pytest.raises(ValueError):
        V.render_drive3d(str(tmp_path / "nothing"), gt)
