"""The paint floor on the GPU (pointnet_refine_amd/paintfloor.py, csrc/prh_floor.hpp) against the
plain-Python oracle (tests/_floor_oracle.py), as bits and integers: the cells and gates of the surface
histogram, blocks that straddle slices, order, dtype and placement, contention on one bin, the
threshold kernel on hand-made rows, the parameter checks, and intensity_floor="auto" end to end."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import _align_cases as AC
import _floor_cases as C
import _floor_oracle as O
from pointnet_refine_amd import paintfloor as PF

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _hist(c, points=None, offsets=None, **more):
    res = PF.surface_histograms(c["points"] if points is None else points, c["slice_offsets"] if offsets is None else offsets,
                                ground=c["ground"], **dict(c["kw"], **more))
    assert res.is_cuda and res.dtype == torch.int64
    return res.cpu().numpy()


def _otsu(rows, min_points=16):
    res = PF.otsu_floors(np.array(rows, dtype=np.int64).reshape(len(rows), -1), min_points)
    assert all(res[k].is_cuda for k in res)
    return {k: v.cpu().numpy() for k, v in res.items()}


# ------------------------------------------------------------------ the histogram kernel
@pytest.mark.parametrize("n_bins", C.GATE_BINS)
def test_cells_and_gates(n_bins):
    """gates_case: cell borders, -half_width, one ulp outside the window, the NaN ground cell, |z - g| at
    the band and beyond, non-finite z, I = -0.0, a tiny negative, NaN, inf, n_bins * bin_width, 1e30;
    bin_width 0.5 with n_bins 2, 64, 65, 256 and 1024."""
    c, want = C.case("gates", n_bins, 0.5), C.expected("gates", n_bins, 0.5)
    assert want.shape == (1, n_bins) and want[0, 0] > 0 and want[0, -1] > 0
    got = _hist(c)
    assert got.shape == want.shape and np.array_equal(got, want), np.flatnonzero(got != want)
    assert np.array_equal(_hist(c, points=c["points"][::-1].copy()), want)


def test_blocks_slices_order_dtype_and_placement():
    """blocks_case: slices of 0, 1, a run minus one, a run, a run plus one and three runs plus five
    points, a block over three slices, a slice with no surface point: the same integers with the points
    shuffled within slices, as float32, from host arrays and device tensors, with 1, 2, 4 and 8 LDS copies."""
    c, want = C.case("blocks"), C.expected("blocks")
    sizes = np.diff(c["slice_offsets"])
    assert sizes.tolist() == list(C.BLOCK_SIZES) and want[2].sum() == 0 and want[3].sum() == 0
    assert all(want[s].sum() > sizes[s] // 2 for s in (0, 4, 5, 6, 7)) and want[:, 40:60].sum() > 1000
    assert np.array_equal(_hist(c), want)
    pts32 = c["points"].astype(np.float32)
    assert np.array_equal(pts32.astype(np.float64), c["points"])
    assert np.array_equal(_hist(c, points=pts32), want)
    dev = PF.surface_histograms(torch.from_numpy(pts32).cuda(), torch.from_numpy(c["slice_offsets"]).cuda(),
                                ground=torch.from_numpy(c["ground"]).cuda())
    assert np.array_equal(dev.cpu().numpy(), want)
    rng = np.random.default_rng(5)
    shuffled = c["points"].copy()
    for a, b in zip(c["slice_offsets"][:-1], c["slice_offsets"][1:]):
        shuffled[a:b] = shuffled[a:b][rng.permutation(b - a)]
    assert np.array_equal(_hist(c, points=shuffled), want)
    for copies in (1, 2, 4, 8):
        assert np.array_equal(_hist(c, copies=copies), want), copies


def test_contention_on_one_bin():
    c = C.case("contention")
    got = _hist(c)
    assert got[0, 7] == 20000 and got.sum() == 20000
    for copies in (1, 2, 4, 8):
        assert np.array_equal(_hist(c, copies=copies), got)


# ------------------------------------------------------------------ the threshold kernel
def test_otsu_pinned_rows_and_rows_without_a_floor():
    for name, (h, min_points, want) in C.PINNED.items():
        got = _otsu([h], min_points)
        assert (got["t_lo"][0], got["t_hi"][0], got["t"][0]) == want, name
        C.same_otsu(got, C.otsu_arrays([h], min_points), name)
        assert got["floor"][0] == float(want[2])
    for name, (h, min_points) in C.NO_FLOOR.items():
        got = _otsu([h], min_points)
        assert (got["t_lo"][0], got["t_hi"][0], got["t"][0]) == (-1, -1, -1) and np.isnan(got["floor"][0]), name
        C.same_otsu(got, C.otsu_arrays([h], min_points), name)


def test_otsu_drive_totals():
    rows = [C.row(64, {3: 2 ** 40, 40: 2 ** 40}), C.row(64, {0: 2 ** 40 + 12345, 63: 2 ** 40 - 1}),
            C.row(64, {10: 2 ** 52 + 1, 11: 3, 50: 2 ** 31}), C.row(64, {5: 2 ** 62 + 2 ** 32, 30: 2 ** 40})]
    got = _otsu(rows)
    C.same_otsu(got, C.otsu_arrays(rows, 16), "2^40")
    assert (got["t_lo"][0], got["t_hi"][0], got["t"][0], got["wr"][0]) == (4, 40, 22, 2 ** 21)


@pytest.mark.parametrize("n_bins", (2, 63, 64, 65, 1024))
def test_otsu_bin_counts(n_bins):
    rng = np.random.default_rng(230 + n_bins)
    rows = C.random_rows(rng, 40, n_bins, top=3000) + [[5] * n_bins, [0] * (n_bins - 1) + [40], [40] + [0] * (n_bins - 1),
                                                         [20] + [0] * (n_bins - 2) + [20]]
    for min_points in (1, 16):
        got = _otsu(rows, min_points)
        C.same_otsu(got, C.otsu_arrays(rows, min_points), f"n_bins {n_bins}")
    assert (got["t"] >= 0).any() and (got["t_lo"][-1], got["t_hi"][-1]) == (1, n_bins - 1)


def test_otsu_0_1_and_300_rows():
    none = PF.otsu_floors(np.zeros((0, 256), dtype=np.int64))
    assert all(none[k].shape == (0,) for k in O.OTSU_KEYS + ("floor",))
    rows = C.random_rows(np.random.default_rng(231), 300, 256, top=400)
    want = C.otsu_arrays(rows, 16)
    C.same_otsu(_otsu(rows), want, "300 rows")
    C.same_otsu(_otsu(rows[:1]), {k: v[:1] for k, v in want.items()}, "1 row")
    dev = PF.otsu_floors(torch.tensor(rows, dtype=torch.int64, device="cuda"))
    C.same_otsu({k: v.cpu().numpy() for k, v in dev.items()}, want, "device rows")


# ------------------------------------------------------------------ parameter checks
def test_bad_parameters_raise_before_any_launch():
    pts, off = np.zeros((3, 4)), np.array([0, 3])
    g = np.zeros((1, 50, 26))
    for kw in (dict(n_bins=1), dict(n_bins=1025), dict(n_bins=2.5), dict(bin_width=0.0), dict(bin_width=float("inf")),
               dict(ground_cell=0.0), dict(ground_cell=0.01), dict(band=-1.0), dict(band=float("nan")), dict(half_length=0.0),
               dict(copies=3)):
        with pytest.raises(ValueError):
            PF.surface_histograms(pts, off, ground=g, **kw)
    with pytest.raises(ValueError):
        PF.surface_histograms(pts, off, ground=np.zeros((1, 50, 25)))
    with pytest.raises(ValueError):
        PF.surface_histograms(np.zeros((3, 3)), off, ground=g)
    with pytest.raises(ValueError):
        PF.surface_histograms(pts, np.array([0, 2]), ground=g)
    with pytest.raises(RuntimeError):
        PF.surface_histograms(torch.zeros((3, 4)), off, ground=g)            # a CPU tensor: there is no CPU path
    for kw in (dict(min_points=0), dict(min_points=1.5), dict(bin_width=-1.0)):
        with pytest.raises(ValueError):
            PF.otsu_floors(np.zeros((1, 8), dtype=np.int64), **kw)
    for shape in ((1, 1), (1, 1025), (8,)):
        with pytest.raises(ValueError):
            PF.otsu_floors(np.zeros(shape, dtype=np.int64))
    with pytest.raises(ValueError):
        PF.paint_floor(pts, off, ground_radius=0.0)
    with pytest.raises(ValueError):                              # no surface point: no floor
        PF.paint_floor(np.zeros((0, 4)), np.zeros(1, dtype=np.int64))
    with pytest.raises(ValueError):
        PF.resolve("automatic", pts, off, "test")
    assert PF.surface_histograms(np.zeros((0, 4)), np.array([0, 0, 0]), ground=np.zeros((2, 50, 26))).tolist() == [[0] * 256] * 2
    # the library checks for itself, before it touches the device
    from pointnet_refine_amd import _lib as L
    lib = L.lib()
    assert lib.prh_floor_max_bins() == PF.MAX_BINS
    hist = torch.zeros((1, 256), dtype=torch.int64, device="cuda")

    def call(half_length=25.0, half_width=12.8, cell=1.0, gx=50, gy=26, band=0.15, bin_width=1.0, n_bins=256, copies=None):
        args = (None, 1, None, 1, 0, half_length, half_width, cell, gx, gy, None, band, bin_width, n_bins, hist.data_ptr(), 0, None)
        return lib.prh_floor_hist(*args) if copies is None else lib.prh_test_floor_hist(copies, *args)

    assert call(gx=0) != 0 and call(gy=1025) != 0 and call(n_bins=1) != 0 and call(n_bins=1025) != 0
    assert call(bin_width=0.0) != 0 and call(bin_width=float("nan")) != 0 and call(band=-0.5) != 0 and call(cell=0.0) != 0
    assert call(half_length=float("inf")) != 0 and call(copies=3) != 0
    assert call() == 0 and call(copies=8) == 0
    outs = [torch.zeros((1,), dtype=d, device="cuda") for d in (torch.int32,) * 3 + (torch.int64,) * 6 + (torch.float64,)]
    ptrs = [o.data_ptr() for o in outs]
    assert lib.prh_floor_otsu(hist.data_ptr(), 1, 1, 16, *ptrs, 0, None) != 0
    assert lib.prh_floor_otsu(hist.data_ptr(), 1, 1025, 16, *ptrs, 0, None) != 0
    assert lib.prh_floor_otsu(hist.data_ptr(), 1, 256, 0, *ptrs, 0, None) != 0
    assert lib.prh_floor_otsu(hist.data_ptr(), -1, 256, 16, *ptrs, 0, None) != 0
    assert lib.prh_floor_otsu(None, 1, 256, 16, *ptrs, 0, None) != 0
    assert lib.prh_floor_otsu(hist.data_ptr(), 1, 256, 16, *ptrs, 0, None) == 0


# ------------------------------------------------------------------ end to end
def _write_drive(root):
    """_align_cases.paint_drive as files: merged.pcd, pose/*.json and a results JSON of the two lanes
    moved by OFFSET in each ego frame."""
    from pointnet_refine_amd.pcd import write_pcd_host
    cloud, poses, pixels = AC.paint_drive()
    drive = root / "drive"
    (drive / "pose").mkdir(parents=True)
    write_pcd_host(str(drive / "merged.pcd"), cloud)
    results = {}
    for k, pose in enumerate(poses):
        ts = 1000 + k
        json.dump({"ts": str(ts), "x": pose[0], "y": pose[1], "z": pose[2], "qx": pose[3], "qy": pose[4], "qz": pose[5],
                   "qw": pose[6]}, open(drive / "pose" / f"{ts}.json", "w"))
        results[f"cam/{ts}.jpg"] = {"pred_instances": [{"data": px.tolist(), "score": 0.9} for px in pixels[k]]}
    json.dump(results, open(root / "results.json", "w"))
    return drive


def _zero_head_model():
    from pointnet_refine_amd.model import LineRefineNet
    from oracle import procedural as P
    m = LineRefineNet()
    m.load_state_dict(P.linerefine_state_dict(0))
    with torch.no_grad():
        for branch in m.reg_branches:
            branch[2].weight.zero_()
            branch[2].bias.zero_()
    return m


FLOOR_KEYS = ("floor", "floor_surface_points", "floor_paint_share", "floor_contrast")


def _same(a, b, what="result"):
    """a and b nested dicts / lists / arrays / scalars: the same structure and the same bytes (NaN equals NaN)."""
    if isinstance(a, dict):
        assert isinstance(b, dict) and sorted(a) == sorted(b), (what, sorted(a), sorted(b))
        for k in a:
            _same(a[k], b[k], f"{what}[{k!r}]")
    elif isinstance(a, (list, tuple)):
        assert len(a) == len(b), what
        for k, (x, y) in enumerate(zip(a, b)):
            _same(x, y, f"{what}[{k}]")
    elif torch.is_tensor(a):
        assert torch.equal(a, b), what
    elif isinstance(a, np.ndarray):
        assert a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes(), what
    else:
        assert a == b or (a != a and b != b), (what, a, b)


def _same_but_floor(auto, fixed):
    """The auto run's report, pieces, fused map, traced lines and support equal the fixed run's, the
    floor* entries of the report left out; returns those."""
    report = dict(auto["report"])
    gained = {k: report.pop(k) for k in FLOOR_KEYS}
    _same(report, fixed["report"], "report")
    for k in ("pieces", "fused", "traced", "support", "piece_slice", "pose_index"):
        assert (k in auto) == (k in fixed), k
        if k in auto:
            _same(auto[k], fixed[k], k)
    return gained


def test_paint_floor_of_the_drive_is_25(tmp_path):
    from pointnet_refine_amd import drive as D
    drive = _write_drive(tmp_path)
    poses = D.load_poses(str(drive / "pose"))
    chosen = D.plan_slices(poses)
    points, offsets, _ = D.slice_cloud(D.load_merged_cloud(str(drive)).astype(np.float32), D.poses_xyzq(poses, chosen),
                                       D.SEGMENT_LEN, D.RADIUS)
    floor, report = PF.paint_floor(points, offsets)
    print(report)
    assert floor == 25.0 and report["floor"] == 25.0 and report["bin"] == 25 and report["plateau"] == (10, 40)
    assert abs(report["paint_share"] - 0.68) <= 0.02 and 40.0 < report["contrast"] < 50.0
    n_s = len(offsets) - 1
    assert report["floor_per_slice"].shape == (n_s,) and report["slices_without_floor"] == 0
    assert (report["floor_per_slice"] == 25.0).all() and 0 < report["surface_points"] <= int(offsets[-1])
    # the pieces: the ground table, then the oracle on the device's own table
    ground = PF.surface_ground(points, offsets)
    assert ground.shape == (n_s, 50, 26) and ground.dtype == torch.float64
    g = ground.cpu().numpy()
    # the disc of an asphalt cell holds about 12 points against ground's min_points of 5, so a few cells fall short
    print("cells with ground among |y| < 3:", float(np.isfinite(g[:, :, 10:16]).mean()))
    assert np.isfinite(g[:, :, 10:16]).mean() > 0.9
    assert np.abs(g[np.isfinite(g)]).max() <= 0.05 and np.isnan(g[:, :, :7]).all()
    hist = PF.surface_histograms(points, offsets, ground=ground).cpu().numpy()
    s = n_s // 2
    a, b = int(offsets[s]), int(offsets[s + 1])
    want = O.surface_histograms(points[a:b].cpu().numpy().astype(np.float64), [0, b - a], g[s:s + 1])
    assert hist[s].tolist() == want[0] and hist.sum() == report["surface_points"]
    assert PF.resolve("auto", points, offsets, "test")[0] == 25.0 and PF.resolve(20.0, points, offsets, "test") == (20.0, None)


def test_refine_cloud_auto_equals_the_floor_it_finds(tmp_path):
    from pointnet_refine_amd import trace as T
    drive = _write_drive(tmp_path)
    model = _zero_head_model().cuda().eval()
    fixed = T.refine_cloud(model, str(drive), intensity_floor=25.0, support=True)
    auto = T.refine_cloud(model, str(drive), intensity_floor="auto", support=True)
    assert not any(k.startswith("floor") for k in fixed["report"])
    gained = _same_but_floor(auto, fixed)
    print(gained)
    assert gained["floor"] == 25.0 and abs(gained["floor_paint_share"] - 0.68) <= 0.02 and gained["floor_surface_points"] > 0
    rep = auto["report"]
    assert all(len(ls) == 2 for ls in auto["traced"]) and rep["trace_lines"] == 2 * rep["slices"] > 0
    assert rep["clusters_kept"] == 2 and len(auto["fused"]) == 2
    for parts in auto["fused"]:                                  # test_trace_gpu's bounds
        xyz = np.concatenate(parts)
        lane = AC.LANE_Y[int(np.argmin([abs(float(xyz[:, 1].mean()) - v) for v in AC.LANE_Y]))]
        print("fused |y - lane| up to", float(np.abs(xyz[:, 1] - lane).max()), " |z| up to", float(np.abs(xyz[:, 2]).max()))
        assert np.abs(xyz[:, 1] - lane).max() <= AC.PAINT_HALF + 1e-4
        assert np.abs(xyz[:, 2]).max() <= 0.05
    with pytest.raises(ValueError):
        T.refine_cloud(model, str(drive), intensity_floor="otsu")


def test_refine_predictions_and_refine_drive_auto(tmp_path):
    from pointnet_refine_amd import fuse as F
    from pointnet_refine_amd import link as LK
    drive = _write_drive(tmp_path)
    model = _zero_head_model().cuda().eval()
    args = (model, str(drive), str(tmp_path / "results.json"))
    fixed = LK.refine_predictions(*args, align=True, support=True, intensity_floor=25.0)
    auto = LK.refine_predictions(*args, align=True, support=True, intensity_floor="auto")
    assert _same_but_floor(auto, fixed)["floor"] == 25.0 and len(auto["fused"]) == 2
    lines = [np.array([[-5.0, y, 0.0], [60.0, y, 0.0], [125.0, y, 0.0]]) for y in AC.LANE_Y]
    fixed = F.refine_drive(model, str(drive), None, lines, support=True, intensity_floor=25.0)
    auto = F.refine_drive(model, str(drive), None, lines, support=True, intensity_floor="auto")
    assert _same_but_floor(auto, fixed)["floor"] == 25.0 and auto["report"]["pieces"] > 0


def test_example_reads_the_floor_and_maps(tmp_path):
    drive = _write_drive(tmp_path)
    ckpt = tmp_path / "model.pth"
    torch.save(_zero_head_model().state_dict(), ckpt)
    out = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "refine_cloud.py"), str(drive), "--checkpoint",
                          str(ckpt), "--out", str(tmp_path / "map.json"), "--intensity-floor", "auto"],
                         capture_output=True, text=True, timeout=300)
    print(out.stdout[-2000:], out.stderr[-2000:])
    assert out.returncode == 0
    assert "PAINT FLOOR  25 " in out.stdout and "PAINT TRACE" in out.stdout and "2 clusters" in out.stdout
