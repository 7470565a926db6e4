"""Paint tracing on the GPU (pointnet_refine_amd/trace.py, csrc/prh_trace.hpp) against the plain-Python
oracle (tests/_trace_oracle.py), as bits: the fixture's designed cases, the compaction of 0 / 1 / 63 /
64 / 65 / 257 peaks per column, ragged slices in any order, dtype, placement and chunking, the
parameter checks, and a lidar drive refined into its two lanes with no detector and no GT."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import _align_cases as AC
import _trace_cases as C
import _trace_oracle as O
from pointnet_refine_amd import trace as T

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DTYPES = {"peak_offsets": torch.int64, "iy": torch.int32, "weight": torch.int64, "count": torch.int32,
          "xyz": torch.float64, "col": torch.int32, "succ": torch.int32, "pred": torch.int32, "bright_points": torch.int64}


def _run(c, points=None, offsets=None, **more):
    res = T.paint_peaks(c["points"] if points is None else points, c["slice_offsets"] if offsets is None else offsets,
                        **dict(c["kw"], **more))
    assert sorted(res) == sorted(DTYPES) and all(res[k].is_cuda and res[k].dtype == DTYPES[k] for k in DTYPES)
    return {k: v.cpu().numpy() for k, v in res.items()}


def _peak_kw(kw):
    return {k: v for k, v in kw.items() if k not in ("min_peaks", "min_length")}


def _case(name):
    c = C.case(name)
    return dict(c, kw=_peak_kw(c["kw"])), O.params(c["kw"])


@pytest.mark.parametrize("name", C.FIXTURE_CASES)
def test_fixture_cases_as_bits(golden_dir, name):
    """cells: points on column / cell borders, at -half_width, one ulp outside, non-finite fields, |z|
    at 512, qi == 0, the weight clamp; peaks: min_points - 1 against min_points, the plateau, cell 0
    and cell ny - 1, nms reaching outside the grid; nms0; links: the tie, the non-mutual pair, tol
    and tol + 1, the gap of max_gap_cols + 1 columns and one more, min_length and just short."""
    g = np.load(os.path.join(golden_dir, "g21_paint_trace.npz"))
    c, p = _case(name)
    assert np.array_equal(C.bits(g[f"{name}_points"]), C.bits(c["points"]))
    want = {k: g[f"{name}_{k}"] for k in DTYPES}
    C.same_bits(_run(c), want, name)
    lines, report = T.trace_lines(c["points"], c["slice_offsets"], p["min_peaks"], p["min_length"], **c["kw"])
    verts, l_off, sl_off = (g[f"{name}_{k}"] for k in ("line_vertices", "line_offsets", "slice_line_offsets"))
    C.same_lines(lines, [[verts[l_off[l]:l_off[l + 1]] for l in range(sl_off[s], sl_off[s + 1])]
                         for s in range(len(sl_off) - 1)], name)
    assert report == {"slices": len(c["slice_offsets"]) - 1, "bright_points": int(want["bright_points"]),
                      "peaks": len(want["iy"]), "links": int((want["succ"] >= 0).sum()), "lines": len(l_off) - 1,
                      "lines_dropped_short": int(g[f"{name}_lines_dropped"])}


def test_compaction_of_0_1_63_64_65_257_peaks_per_column():
    c, _ = _case("compaction")
    want = C.expected("compaction")[0]
    assert np.diff(want["peak_offsets"]).tolist() == [0, 1, 63, 64, 65, 257]
    C.same_bits(_run(c), want, "compaction")


def test_ragged_slices_order_dtype_placement_and_chunks():
    """An empty slice, a slice with no bright point, a one-point slice among painted ones: the same
    bits with the points shuffled within their slices, as float32 of equal value, from the host or
    from the device, and with one slice per chunk."""
    c, p = _case("ragged")
    pts32 = c["points"].astype(np.float32)
    c32 = dict(c, points=pts32.astype(np.float64))               # every value a float32 value
    peaks = O.paint_peaks(c32["points"], c["slice_offsets"], **c["kw"])
    want = C.as_arrays(peaks)
    per_slice = np.add.reduceat(np.diff(want["peak_offsets"]), np.arange(7) * 100)
    assert per_slice[[1, 2, 3, 5]].tolist() == [0, 0, 0, 0] and (per_slice[[0, 4, 6]] > 40).all()
    C.same_bits(_run(c32), want, "float64")
    C.same_bits(_run(c32, points=pts32), want, "float32")
    C.same_bits(_run(c32, points=torch.from_numpy(pts32).cuda(), offsets=torch.from_numpy(c["slice_offsets"]).cuda()),
                want, "device inputs")
    rng = np.random.default_rng(5)
    shuffled = c32["points"].copy()
    for a, b in zip(c["slice_offsets"][:-1], c["slice_offsets"][1:]):
        shuffled[a:b] = shuffled[a:b][rng.permutation(b - a)]
    C.same_bits(_run(c32, points=shuffled), want, "shuffled")
    one = 100 * 512 * T.CELL_BYTES                                # the tables of one slice
    assert T.TABLE_BYTES // one > 7
    for table_bytes in (one, 3 * one, 1):
        C.same_bits(_run(c32, table_bytes=table_bytes), want, f"table_bytes = {table_bytes}")
    lines, _ = T.trace_lines(c32["points"], c["slice_offsets"], table_bytes=one, **c["kw"])
    C.same_lines(lines, [[np.array(l) for l in ls] for ls in O.chain_lines(peaks, 7, 100)[0]], "ragged lines")
    assert [len(ls) for ls in lines] == [2, 0, 0, 0, 2, 0, 2]


def test_empty_inputs_and_bad_parameters_raise_before_any_launch():
    none = T.paint_peaks(np.zeros((0, 4)), np.zeros(1, dtype=np.int64))
    assert none["peak_offsets"].tolist() == [0] and none["iy"].shape == (0,) and none["xyz"].shape == (0, 3)
    lines, report = T.trace_lines(np.zeros((0, 4)), np.array([0, 0, 0]))
    assert lines == [[], []] and report["peaks"] == 0 and report["slices"] == 2
    pts, off = np.zeros((3, 4)), np.array([0, 3])
    for kw in (dict(cell=0.0), dict(cell=-1.0), dict(cell=0.005), dict(intensity_floor=float("nan")), dict(nms=-1)):
        with pytest.raises(ValueError):
            T.paint_peaks(pts, off, **kw)
    with pytest.raises(ValueError):
        T.paint_peaks(np.zeros((3, 3)), off)
    with pytest.raises(ValueError):
        T.paint_peaks(pts, np.array([0, 2]))
    with pytest.raises(RuntimeError):
        T.paint_peaks(torch.zeros((3, 4)), off)                  # a CPU tensor: there is no CPU path
    # the library checks for itself, before it touches the device
    from pointnet_refine_amd import _lib as L
    lib = L.lib()
    assert lib.prh_trace_workspace_bytes(1, 100, 4097) == 0 and lib.prh_trace_workspace_bytes(1, 100, 512) >= 100 * 512 * 36
    assert lib.prh_trace_max_nms() == T.MAX_NMS
    ws = torch.zeros(lib.prh_trace_workspace_bytes(1, 8, 16), dtype=torch.uint8, device="cuda")
    args = (None, 1, None, 1, 0, 0, 2.0, 0.5, 8, 0.5)
    tail = (ws.data_ptr(), ws.numel(), 0, None)
    assert lib.prh_trace_hist(*args, 0.0, 16, 0.0, *tail) != 0
    assert lib.prh_trace_hist(*args, 0.0625, 4097, 0.0, *tail) != 0
    assert lib.prh_trace_hist(*args, 0.0625, 16, float("nan"), *tail) != 0
    assert lib.prh_trace_hist(*args, 0.0625, 16, 0.0, ws.data_ptr(), 64, 0, None) != 0
    assert lib.prh_trace_peaks_count(ws.data_ptr(), ws.numel(), 1, 8, 16, -1, 3, 1, None, 0, None) != 0
    assert lib.prh_trace_hist(*args, 0.0625, 16, 0.0, *tail) == 0


# ------------------------------------------------------------------ a lidar drive with no detector
def _write_drive(root):
    """_align_cases.paint_drive as files, with no results file: merged.pcd and pose/*.json."""
    from pointnet_refine_amd.pcd import write_pcd_host
    cloud, poses, _ = AC.paint_drive()
    drive = root / "drive"
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


def _same_map(a, b):
    assert a["report"] == b["report"] and a["pieces"].tobytes() == b["pieces"].tobytes()
    assert len(a["fused"]) == len(b["fused"])
    assert all(len(p) == len(q) and all(x.tobytes() == y.tobytes() for x, y in zip(p, q))
               for p, q in zip(a["fused"], b["fused"]))


def test_refine_cloud_maps_the_drive_without_a_detector(tmp_path):
    drive = _write_drive(tmp_path)
    assert not (tmp_path / "results.json").exists()
    model = _zero_head_model().cuda().eval()
    res = T.refine_cloud(model, str(drive), intensity_floor=20.0)
    rep = res["report"]
    print(rep)
    assert rep["trace_slices"] == rep["slices"] == len(res["traced"]) == len(res["pose_index"]) > 0
    assert all(len(ls) == 2 for ls in res["traced"]) and rep["trace_lines"] == 2 * rep["slices"]
    assert rep["clusters_kept"] == 2 and len(res["fused"]) == 2
    for parts in res["fused"]:
        xyz = np.concatenate(parts)
        lane = AC.LANE_Y[int(np.argmin([abs(float(xyz[:, 1].mean()) - v) for v in AC.LANE_Y]))]
        print("fused |y - lane| up to", float(np.abs(xyz[:, 1] - lane).max()), " |z| up to", float(np.abs(xyz[:, 2]).max()))
        assert np.abs(xyz[:, 1] - lane).max() <= AC.PAINT_HALF + 1e-4      # 1e-4: test_link_gpu's fp32 path bound
        assert np.abs(xyz[:, 2]).max() <= 0.05                            # test_ground_gpu's bound for this cloud
    _same_map(T.refine_cloud(model, str(drive), intensity_floor=20.0, batched=True), res)
    _same_map(T.refine_cloud(model, str(drive), intensity_floor=20.0, device_sync=True), res)


def test_example_traces_and_maps(tmp_path):
    drive = _write_drive(tmp_path)
    ckpt = tmp_path / "model.pth"
    torch.save(_zero_head_model().state_dict(), ckpt)
    out = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "refine_cloud.py"), str(drive), "--checkpoint",
                          str(ckpt), "--out", str(tmp_path / "map.json"), "--intensity-floor", "20"],
                         capture_output=True, text=True, timeout=300)
    print(out.stdout[-2000:], out.stderr[-2000:])
    assert out.returncode == 0
    assert "PAINT TRACE" in out.stdout and "2 clusters" in out.stdout
