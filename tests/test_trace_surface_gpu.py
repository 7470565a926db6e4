"""The surface gate of paint tracing on the GPU (pointnet_refine_amd/trace.py, csrc/prh_trace.hpp) against
the plain-Python oracle (tests/_trace_surface_oracle.py) and against the ungated kernel on the rows the
oracle keeps, as bits: designed points, ragged slices in any order, dtype, placement and chunking, the
band's extremes, the floor from a prebuilt table, and a drive with a bright trail above the road that is
traced without the gate and gone with it."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import _align_cases as AC
import _trace_cases as C
import _trace_surface_cases as SC
import _trace_surface_oracle as SO
from pointnet_refine_amd import paintfloor as PF
from pointnet_refine_amd import trace as T

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KEYS = C.KEYS + ("bright_points",)


def _run(case, points=None, ground="case", **more):
    kw = {k: v for k, v in case["kw"].items() if not k.startswith("g_")}
    res = T.paint_peaks(case["points"] if points is None else points, case["slice_offsets"],
                        ground=case["ground"] if isinstance(ground, str) else ground, **dict(kw, **more))
    assert ("off_surface" in res) == (ground is not None)
    if ground is not None:
        assert res["off_surface"].dtype == torch.int64 and res["off_surface"].shape == (len(case["slice_offsets"]) - 1,)
    return {k: v.cpu().numpy() for k, v in res.items()}


def _same(got, want, what):
    """Every array of paint_peaks and off_surface equal the oracle's, as bits."""
    C.same_bits(got, C.as_arrays(want), what)
    assert got["off_surface"].tolist() == want["off_surface"], (what, got["off_surface"].tolist(), want["off_surface"])


def _placed(points, dtype):
    """points as a CUDA tensor that begins 16 bytes into a larger buffer."""
    lead = 16 // torch.empty((), dtype=dtype).element_size()
    buf = torch.full((lead + points.size + 8,), float("nan"), dtype=dtype, device="cuda")
    view = buf[lead:lead + points.size].view(-1, 4)
    view.copy_(torch.from_numpy(points).to(dtype))
    assert view.data_ptr() == buf.data_ptr() + 16
    return view


def test_designed_points_float64_and_float32():
    case, want_off, _ = SC.designed_case()
    want = SO.paint_peaks(case["points"], case["slice_offsets"], case["ground"], **case["kw"])
    assert want["off_surface"] == want_off
    _same(_run(case), want, "float64")
    c32 = SC.as_float32_values(case)
    want32 = SO.paint_peaks(c32["points"], case["slice_offsets"], case["ground"], **case["kw"])
    assert want32["off_surface"] != want_off                     # the one-ulp points are float64 points
    _same(_run(c32, points=c32["points"].astype(np.float32)), want32, "float32")
    _same(_run(c32), want32, "float32 values as float64")
    _same(_run(case, ground=torch.from_numpy(case["ground"]).cuda()), want, "a CUDA table")


def test_a_narrower_ground_window_at_the_c_abi():
    """trace.paint_peaks ties the ground window to the trace window; the library does not.  With a
    ground window of half length 3 under the trace grid of half length 4 the points at x = +-3.5 are off
    the surface: the table of counts and off_surface against the oracle."""
    from pointnet_refine_amd import _lib as L
    import _trace_oracle as O
    case, _, _ = SC.designed_case()
    ground = np.zeros((2, 6, 4))
    want = SO.paint_peaks(case["points"], case["slice_offsets"], ground, g_half_length=3.0, **case["kw"])
    lib, p = L.lib(), case["kw"]
    pts, off = torch.from_numpy(case["points"]).cuda(), torch.from_numpy(case["slice_offsets"]).cuda()
    gt, counted = torch.from_numpy(ground).cuda(), torch.full((2,), -1, dtype=torch.int64, device="cuda")
    nb = lib.prh_trace_workspace_bytes(2, 16, 64)
    ws = torch.empty((nb,), dtype=torch.uint8, device="cuda")
    args = (pts.data_ptr(), 1, off.data_ptr(), 2, 0, len(case["points"]), p["half_length"], p["col"], 16, p["half_width"],
            p["cell"], 64, p["intensity_floor"], ws.data_ptr(), nb)
    gate = (3.0, p["half_width"], 1.0, 6, 4, gt.data_ptr(), p["band"], counted.data_ptr(), 0, None)
    L.check(lib.prh_trace_hist_surface(*args, *gate), "prh_trace_hist_surface")
    n = ws[:4 * 2 * 16 * 64].view(torch.int32).view(2, 16, 64).cpu().numpy()
    assert counted.tolist() == want["off_surface"] == [8, 1]
    kept = case["points"][np.array(want["keep"])]
    new_off = np.cumsum([0, 15 - 8, 2 - 1])
    for s in range(2):
        tab, bright = O.slice_tables(kept[new_off[s]:new_off[s + 1]], O.params({k: v for k, v in p.items() if k != "band"}), 16, 64)
        dense = np.zeros((16, 64), dtype=np.int32)
        for (ix, iy), t in tab.items():
            dense[ix, iy] = t[0]
        assert np.array_equal(n[s], dense) and int(n[s].sum()) == bright
    # the library checks the gate's parameters for itself, before it touches the device
    for bad in ((3.0, 2.0, 1.0, 0, 4), (3.0, 2.0, 1.0, 6, 1025), (0.0, 2.0, 1.0, 6, 4), (3.0, 2.0, float("nan"), 6, 4)):
        assert lib.prh_trace_hist_surface(*args, *bad, *gate[5:]) != 0
    for band in (-0.125, float("nan"), float("inf")):
        assert lib.prh_trace_hist_surface(*args, *gate[:6], band, *gate[7:]) != 0
    assert lib.prh_trace_hist_surface(*args, *gate[:5], None, *gate[6:]) != 0
    assert lib.prh_trace_hist_surface(*args, *gate[:7], None, 0, None) != 0
    assert lib.prh_trace_hist_surface(*args, *gate) == 0


def test_ragged_slices_order_dtype_placement_and_chunks():
    """Slices of 0, 1, 257 and 5,000 shuffled points, a third of the bright ones off the surface: the
    oracle's bits, and the bits of the ungated paint_peaks on the rows the oracle's mask keeps - the
    kernel that was there before the gate - as float64 and float32, placed 16 bytes into a larger buffer,
    with one slice per chunk and with all slices in one."""
    case, want = SC.ragged_case()
    keep = np.array(want["keep"])
    off = case["slice_offsets"]
    kept_off = np.cumsum([0] + [int(keep[a:b].sum()) for a, b in zip(off[:-1], off[1:])]).astype(np.int64)
    assert kept_off[-1] == keep.sum() and kept_off.tolist()[:3] == [0, 0, 0]
    ungated = {k: v.cpu().numpy() for k, v in T.paint_peaks(case["points"][keep], kept_off, **case["kw"]).items()}
    C.same_bits(ungated, C.as_arrays(want), "the ungated kernel on the kept rows")
    one = 32 * 128 * T.CELL_BYTES                                 # the tables of one slice
    assert T.TABLE_BYTES // one > 4
    for dtype in (torch.float64, torch.float32):
        placed = _placed(case["points"], dtype)
        for table_bytes in (one, T.TABLE_BYTES):
            got = _run(case, points=placed, table_bytes=table_bytes)
            _same(got, want, f"{dtype}, table_bytes = {table_bytes}")
            C.same_bits(got, ungated, f"{dtype}, table_bytes = {table_bytes}: against the ungated kernel")
    _same(_run(case), want, "from the host")
    no_gate = _run(case, ground=None)
    assert int(no_gate["bright_points"]) == int(want["bright_points"]) + sum(want["off_surface"])


def test_band_zero_and_a_table_without_ground():
    case, want = SC.ragged_case()
    # band 0: a point exactly at its cell's height is kept, every other bright point is off the surface
    pts = case["points"].copy()
    bright = np.flatnonzero(pts[:, 3] > 20.0)
    exact = bright[::3]
    s_of = np.searchsorted(case["slice_offsets"], exact, side="right") - 1
    g = case["ground"][s_of, np.clip(np.floor(pts[exact, 0] + 8.0), 0, 15).astype(int),
                       np.clip(np.floor(pts[exact, 1] + 4.0), 0, 7).astype(int)]
    pts[exact, 2] = np.nan_to_num(g, nan=1.0)
    zero = SO.paint_peaks(pts, case["slice_offsets"], case["ground"], band=0.0, **case["kw"])
    inside = (np.abs(pts[exact, 0]) < 8.0) & (np.abs(pts[exact, 1]) < 4.0) & np.isfinite(g)
    assert zero["bright_points"] >= inside.sum() > 100
    _same(_run(dict(case, points=pts), band=0.0), zero, "band 0")
    # no ground anywhere: no peak, and every bright point of the ungated run is off the surface
    nothing = _run(case, ground=np.full(case["ground"].shape, np.nan))
    assert nothing["iy"].shape == (0,) and int(nothing["bright_points"]) == 0 and not nothing["peak_offsets"].any()
    assert int(nothing["off_surface"].sum()) == int(_run(case, ground=None)["bright_points"]) > 1000
    with pytest.raises(RuntimeError):
        T.paint_peaks(case["points"], case["slice_offsets"], ground=torch.from_numpy(case["ground"]), **case["kw"])


# ------------------------------------------------------------------ a drive with a trail above the road
ROAD_Z, TRAIL_UP, TRAIL_I, FLOOR = 0.5, 0.6, 200.0, 20.0


def _clouds():
    """Drive A: two painted lanes (intensity 40-60) on asphalt dense enough for every ground cell, the
    road at z = 0.5.  Drive B: A and a trail along y = 0, 0.6 m above the road, a point every 0.125 m,
    four times as bright as the paint: four points per 0.5 m column, a dozen in a ground cell's disc
    that holds about 35 road points, so the road height of no cell moves."""
    rng = np.random.default_rng(231)
    a = AC.paint_cloud(rng, -8.0, 128.0, asphalt_per_m2=20.0, z=ROAD_Z)
    x = np.arange(-8.0, 128.0, 0.125)
    trail = np.column_stack([x, rng.uniform(-0.01, 0.01, len(x)), ROAD_Z + TRAIL_UP + rng.normal(0.0, 0.02, len(x)),
                             np.full(len(x), TRAIL_I)])
    poses = AC.paint_drive()[1]
    return a.astype(np.float32), np.concatenate([a, trail]).astype(np.float32), poses


def _write_drive(root, name, cloud, poses):
    from pointnet_refine_amd.pcd import write_pcd_host
    drive = root / name
    (drive / "pose").mkdir(parents=True)
    write_pcd_host(str(drive / "merged.pcd"), cloud)
    for k, pose in enumerate(poses):
        ts = 1000 + k
        json.dump({"ts": str(ts), "x": pose[0], "y": pose[1], "z": pose[2], "qx": pose[3], "qy": pose[4], "qz": pose[5],
                   "qw": pose[6]}, open(drive / "pose" / f"{ts}.json", "w"))
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


def _slices(cloud, poses):
    from pointnet_refine_amd import drive as D
    return D.slice_cloud(cloud, np.asarray(poses, dtype=np.float64)[D.plan_slices(poses)], D.SEGMENT_LEN, D.RADIUS)[:2]


def _same_lines(a, b):
    return len(a) == len(b) and all(len(p) == len(q) and all(x.tobytes() == y.tobytes() for x, y in zip(p, q))
                                    for p, q in zip(a, b))


def test_paint_floor_with_a_prebuilt_table():
    cloud_a, _, poses = _clouds()
    points, offsets = _slices(cloud_a, poses)
    floor, report = PF.paint_floor(points, offsets)
    table = PF.surface_ground(points, offsets)
    floor_t, report_t = PF.paint_floor(points, offsets, ground=table)
    assert floor == floor_t and sorted(report) == sorted(report_t)
    for k, v in report.items():
        assert np.array_equal(v, report_t[k], equal_nan=True) if isinstance(v, np.ndarray) else v == report_t[k], k
    assert PF.resolve("auto", points, offsets, "test", table)[0] == floor == PF.paint_floor(points, offsets, table.cpu().numpy())[0]
    with pytest.raises(ValueError):
        PF.paint_floor(points, offsets, ground=table[1:])
    with pytest.raises(ValueError):
        PF.paint_floor(points, offsets, ground=table, half_width=6.4)


def test_the_trail_is_traced_without_the_gate_and_gone_with_it(tmp_path):
    cloud_a, cloud_b, poses = _clouds()
    pts_a, off_a = _slices(cloud_a, poses)
    pts_b, off_b = _slices(cloud_b, poses)
    # the premise: the trail is too sparse to move the road height of any cell
    assert torch.equal(PF.surface_ground(pts_a, off_a).view(torch.int64), PF.surface_ground(pts_b, off_b).view(torch.int64))
    pb = pts_b.cpu().numpy()
    trail = int(((pb[:, 3] == TRAIL_I) & (pb[:, 0] >= -25.0) & (pb[:, 0] < 25.0) & (np.abs(pb[:, 1]) < 12.8)).sum())
    assert trail > 4 * 100 * len(off_b[:-1]) // 2

    model = _zero_head_model().cuda().eval()
    a = T.refine_cloud(model, cloud_a, poses, intensity_floor=FLOOR)
    a_s = T.refine_cloud(model, cloud_a, poses, intensity_floor=FLOOR, surface=True)
    b = T.refine_cloud(model, cloud_b, poses, intensity_floor=FLOOR)
    b_s = T.refine_cloud(model, cloud_b, poses, intensity_floor=FLOOR, surface=True)
    n_s = a["report"]["slices"]
    print({k: r["report"]["trace_lines"] for k, r in (("A", a), ("A surface", a_s), ("B", b), ("B surface", b_s))},
          "trail points", trail, "off the surface", b_s["report"]["trace_off_surface_points"])
    assert n_s == len(off_a) - 1 > 0 and all(len(ls) == 2 for ls in a["traced"]) and len(a["fused"]) == 2
    # B at the default: the trail is a third line in every slice and in the map
    assert not _same_lines(b["traced"], a["traced"])
    assert all(len(ls) == 3 for ls in b["traced"]) and len(b["fused"]) == 3
    assert "trace_off_surface_points" not in b["report"] and "trace_surface_band" not in b["report"]
    # B with the gate: what A gives with the gate, bit for bit, and the trail counted
    assert _same_lines(b_s["traced"], a_s["traced"])
    assert all(len(ls) == 2 for ls in b_s["traced"]) and len(b_s["fused"]) == 2
    assert b_s["report"]["trace_off_surface_points"] == trail and b_s["report"]["trace_surface_band"] == PF.BAND
    # A with the gate: nothing on this road is off the surface, so nothing changes
    assert _same_lines(a_s["traced"], a["traced"]) and a_s["report"]["trace_off_surface_points"] == 0
    assert a_s["pieces"].tobytes() == a["pieces"].tobytes()
    gained = {k: v for k, v in a_s["report"].items() if k not in a["report"]}
    assert gained == {"trace_surface_band": PF.BAND, "trace_off_surface_points": 0}
    assert {k: v for k, v in a_s["report"].items() if k in a["report"]} == a["report"]
    # one table for the gate and the floor: the floor "auto" finds is the one it finds alone
    auto = T.refine_cloud(model, cloud_b, poses, intensity_floor="auto", surface=True)
    assert auto["report"]["floor"] == T.refine_cloud(model, cloud_b, poses, intensity_floor="auto")["report"]["floor"]
    assert all(len(ls) == 2 for ls in auto["traced"]) and auto["report"]["trace_off_surface_points"] == trail
    for band in (-0.1, float("nan")):
        with pytest.raises(ValueError):
            T.refine_cloud(model, cloud_b, poses, intensity_floor=FLOOR, surface=True, surface_band=band)


def test_example_with_the_gate(tmp_path):
    _, cloud_b, poses = _clouds()
    drive = _write_drive(tmp_path, "drive_b", cloud_b, poses)
    ckpt = tmp_path / "model.pth"
    torch.save(_zero_head_model().state_dict(), ckpt)
    out = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "refine_cloud.py"), str(drive), "--checkpoint",
                          str(ckpt), "--out", str(tmp_path / "map.json"), "--intensity-floor", "auto", "--surface"],
                         capture_output=True, text=True, timeout=300)
    print(out.stdout[-2000:], out.stderr[-2000:])
    assert out.returncode == 0
    lines = [l for l in out.stdout.splitlines() if l.startswith("PAINT TRACE")]
    assert len(lines) == 1 and lines[0].endswith(" bright points off the surface") and "2 clusters" in out.stdout
    assert int(lines[0].split("   ")[-1].split()[0]) > 0 and "PAINT FLOOR" in out.stdout
    from pointnet_refine_amd import drive as D
    assert "Wrote 2 polylines" in out.stdout and len(D.load_gt_items(str(tmp_path / "map.json"))) == 2
