"""Cloud support on the GPU (csrc/prh_support.hpp through pointnet_refine_amd.support) against the
restatement of the rule in _support_oracle.py, which walks every segment for every point and knows
no grid: the stored fixture, shapes chosen to break the kernel, independence of the grid, of the
order of the points and of how the cloud is split, empty inputs, and a painted drive end to end.

The sums are integers and are compared for equality.  That is well-posed because every exact case
first asserts the oracle's margins (_support_cases.assert_margins): |d2 - r2| >= 1e-9 m^2 for every
(point, line) pair, s / step + 0.5 at least 1e-9 from an integer for every hit not clamped to the
last node, and t * 65536, hz * 65536, wI * 256 at least 1e-8 from a half-integer.  Device and
oracle run the same IEEE operations; a last-bit difference in a sqrt or a division is about 4e-12
of a quantum at t = 0.3, three to four orders below the margins."""
import os

import numpy as np
import pytest
import torch

import _support_cases as C
import _support_oracle as O
from pointnet_refine_amd import fuse as F
from pointnet_refine_amd import support as S

pytestmark = pytest.mark.gpu


def _equal(got, want_acc, want_off):
    print("acc equal:", np.array_equal(got["acc"], want_acc), "hits gpu / oracle:", int(got["acc"][:, 0].sum()),
          int(want_acc[:, 0].sum()), "differing rows:", int((got["acc"] != want_acc).any(1).sum()) if
          got["acc"].shape == want_acc.shape else "shape")
    assert got["acc"].dtype == np.int64 and got["acc"].shape == want_acc.shape
    assert np.array_equal(got["offsets"], want_off)
    assert np.array_equal(got["acc"], want_acc)


def test_fixture(golden_dir):
    g = np.load(os.path.join(golden_dir, "g17_cloud_support.npz"))
    off = g["line_offsets"]
    lines = [g["line_vertices"][off[l]:off[l + 1]] for l in range(len(off) - 1)]
    r = O.support(g["cloud"], lines, float(g["step"]), float(g["radius"]), float(g["intensity_floor"]))
    C.assert_margins(r["margins"])
    assert np.array_equal(r["acc"], g["acc"])                      # the stored result is the rule's
    got = S.node_support(g["cloud"], lines, float(g["step"]), float(g["radius"]), float(g["intensity_floor"]))
    assert np.array_equal(got["origin"], g["origin"])
    _equal(got, g["acc"], g["node_offsets"])


@pytest.mark.parametrize("radius", [0.3, 1.0])
@pytest.mark.parametrize("step", [0.5, 0.37])
@pytest.mark.parametrize("size", C.SIZES)
def test_shapes(size, step, radius):
    lines, cloud = C.shapes_case()
    r = C.shapes_oracle(step, radius)
    C.assert_margins(r["margins"])
    want = O.accumulate(r["hits"], len(r["acc"]), size)
    got = S.node_support(cloud[:size], lines, step, radius, C.FLOOR)
    _equal(got, want, r["offsets"])
    if size == C.SIZES[-1]:
        off, n = got["offsets"], got["n"]
        assert off[3] - off[2] == 1 and n[off[2]] == 0             # all vertices equal: one node, never a hit
        assert off[4] - off[3] == 1 and n[off[3]] > 0              # shorter than the step: one node takes every hit
        assert all(n[off[l]:off[l + 1]].sum() > 0 for l in (0, 1, 4, 5, 6, 7, 8, 9))
        per_point = np.bincount([i for i, *_ in r["hits"]], minlength=size)
        assert per_point.max() >= 2                                # a point in two tubes counts for both
        assert got["acc"][:, 7].max() == 0 and got["acc"][:, 1].sum() < got["acc"][:, 0].sum()
        assert np.isnan(got["offset"][n == 0]).all() and np.isfinite(got["offset"][n > 0]).all()


def test_grid_independence(monkeypatch):
    lines, cloud = C.shapes_case()
    r = C.shapes_oracle(0.5, 1.0)
    C.assert_margins(r["margins"])
    for cell in (1.0, 4.0, 64.0):
        got = S.node_support(cloud, lines, 0.5, 1.0, C.FLOOR, cell=cell)
        assert got["acc"].tobytes() == r["acc"].tobytes(), cell
    monkeypatch.setattr(S, "MAX_CELLS", 16)                         # the automatic cap: cells grow until 16 are left
    shifted = [l - r["origin"] for l in lines]
    grid = S.segment_grid(shifted, 1.0, 1.0)
    assert grid["nx"] * grid["ny"] <= 16 and grid["cell"] > 4.0
    got = S.node_support(cloud, lines, 0.5, 1.0, C.FLOOR, cell=1.0)
    assert got["acc"].tobytes() == r["acc"].tobytes()
    monkeypatch.undo()
    # two lines 5,000 km apart: the cap acts on its own and the near line's rows do not change
    far = lines + [lines[0] + [5.0e6, 5.0e6, 0.0]]
    assert S.segment_grid([l - r["origin"] for l in far], 1.0, 4.0)["cell"] > 1000.0
    got = S.node_support(cloud, far, 0.5, 1.0, C.FLOOR, origin=r["origin"])
    n0 = len(r["acc"])
    assert got["acc"][:n0].tobytes() == r["acc"].tobytes() and got["acc"][n0:].max() == 0


def test_order_additivity_and_repeats():
    lines, cloud = C.shapes_case()
    r = C.shapes_oracle(0.5, 0.3)
    a = S.node_support(cloud, lines, 0.5, 0.3, C.FLOOR)
    b = S.node_support(cloud, lines, 0.5, 0.3, C.FLOOR)
    for k in a:
        assert np.asarray(a[k]).tobytes() == np.asarray(b[k]).tobytes(), k          # two runs
    assert a["acc"].tobytes() == r["acc"].tobytes()
    perm = np.random.default_rng(3).permutation(len(cloud))
    assert S.node_support(cloud[perm], lines, 0.5, 0.3, C.FLOOR)["acc"].tobytes() == a["acc"].tobytes()
    half = perm[:1400]
    rest = perm[1400:]
    parts = [S.node_support(cloud[ix], lines, 0.5, 0.3, C.FLOOR)["acc"] for ix in (half, rest)]
    assert np.array_equal(parts[0] + parts[1], a["acc"])
    on_device = torch.from_numpy(cloud).cuda()
    t = S.node_support(on_device, lines, 0.5, 0.3, C.FLOOR)
    assert t["acc"].tobytes() == a["acc"].tobytes()
    assert S.node_support(on_device[1:], lines, 0.5, 0.3, C.FLOOR)["acc"][:, 0].sum() == a["acc"][:, 0].sum() - 1


def test_empty_inputs():
    lines, cloud = C.shapes_case()
    r = C.shapes_oracle(0.5, 0.3)
    none = S.node_support(np.zeros((0, 4), dtype=np.float32), lines)
    assert none["acc"].shape == r["acc"].shape and none["acc"].max() == 0 and np.array_equal(none["offsets"], r["offsets"])
    assert np.isnan(none["offset"]).all() and none["n"].sum() == 0
    no_lines = S.node_support(cloud, [])
    assert no_lines["acc"].shape == (0, 8) and np.array_equal(no_lines["offsets"], [0])
    bare = S.node_support(cloud, [np.zeros((0, 3)), lines[0], np.zeros((0, 3))], 0.5, 0.3, C.FLOOR, origin=r["origin"])
    n0 = int(r["offsets"][1])
    assert np.array_equal(bare["offsets"], [0, 0, n0, n0]) and bare["acc"].tobytes() == r["acc"][:n0].tobytes()
    only_bare = S.node_support(cloud, [np.zeros((0, 3))])
    assert only_bare["acc"].shape == (0, 8) and np.array_equal(only_bare["offsets"], [0, 0])
    one_vertex = S.node_support(cloud, [lines[0][:1]])
    assert one_vertex["acc"].shape == (1, 8) and one_vertex["acc"].max() == 0
    m = S.map_support(cloud, [])
    assert m["nodes"] == 0 and m["points"] == 0 and np.isnan(m["offset_w_mean"]) and S.marking_attributes(m) == []


# ------------------------------------------------------------------ the painted drive, end to end
def _zero_head_model():
    from pointnet_refine_amd.model import LineRefineNet
    from oracle import procedural as P
    m = LineRefineNet()
    m.load_state_dict(P.linerefine_state_dict(0))
    with torch.no_grad():
        for branch in m.reg_branches:
            branch[2].weight.zero_()
            branch[2].bias.zero_()
    return m.cuda().eval()


def test_painted_drive_end_to_end():
    """Paint 0.1 m to the right of the lines handed in: a uniform stripe of half-width 0.075 m has
    sigma = 0.043 m per point and every line has at least 600 paint points, so the standard error of
    the weighted offset is about 0.002 m; 0.02 m is ten of them."""
    poses, cloud, lines = C.painted_drive()
    moved = [l + [0.0, 0.1, 0.0] for l in lines]
    model = _zero_head_model()
    res = F.refine_drive(model, cloud, poses, moved, support=True, intensity_floor=20.0)
    sup = res["support"]
    print("offset_w_mean input / fused:", sup["input"]["offset_w_mean"], sup["fused"]["offset_w_mean"], "markings:",
          [a["marking"] for a in sup["attributes"]], "painted shares:", [a["painted_share"] for a in sup["attributes"]])
    assert [a["marking"] for a in sup["attributes"]] == ["solid", "dashed", "none"]
    assert abs(sup["input"]["offset_w_mean"] + 0.1) <= 0.02 and abs(sup["fused"]["offset_w_mean"] + 0.1) <= 0.02
    for l in (0, 1):
        assert abs(sup["fused"]["per_line"][l]["offset_w_mean"] + 0.1) <= 0.02
        assert sup["attributes"][l]["runs"] >= (1 if l == 0 else 2)
    assert sup["fused"]["supported_share"] > 0.9 and sup["input"]["supported_share"] < sup["fused"]["supported_share"]
    on = S.map_support(cloud, lines, intensity_floor=20.0)
    print("offset_w_mean on the unshifted lines:", on["offset_w_mean"])
    assert abs(on["offset_w_mean"]) <= 0.02
    plain = F.refine_drive(model, cloud, poses, moved)
    assert "support" not in plain
    assert set(plain) == {"fused", "pieces", "piece_line", "piece_slice", "pose_index", "poses", "nodes", "report"}
    assert set(res) == set(plain) | {"support"}
    assert all(x.tobytes() == y.tobytes() for p, q in zip(plain["fused"], res["fused"]) for x, y in zip(p, q))


def test_example_scores_the_painted_drive(tmp_path):
    import json
    import subprocess
    import sys
    from pointnet_refine_amd.pcd import write_pcd_host
    poses, cloud, lines = C.painted_drive()
    drive = tmp_path / "drive"
    (drive / "pose").mkdir(parents=True)
    for k, p in enumerate(poses):
        json.dump({"ts": str(1000 + k), "x": p[0], "y": p[1], "z": p[2], "qx": p[3], "qy": p[4], "qz": p[5], "qw": p[6]},
                  open(drive / "pose" / f"{1000 + k}.json", "w"))
    write_pcd_host(str(drive / "merged.pcd"), cloud.astype(np.float64))
    F.write_map_json(str(tmp_path / "lines.json"), [[l + [0.0, 0.1, 0.0]] for l in lines], categories=["lane"] * 3)
    ckpt = tmp_path / "model.pth"
    torch.save(_zero_head_model().cpu().state_dict(), ckpt)
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out = subprocess.run([sys.executable, os.path.join(root, "examples", "refine_drive.py"), str(drive),
                          str(tmp_path / "lines.json"), "--checkpoint", str(ckpt), "--out", str(tmp_path / "map.json"),
                          "--support", "--intensity-floor", "20"], capture_output=True, text=True, timeout=300)
    print(out.stdout[-2000:], out.stderr[-2000:])
    assert out.returncode == 0
    line = [ln for ln in out.stdout.splitlines() if ln.startswith("MAP SUPPORT")]
    assert len(line) == 1 and "1 solid, 1 dashed, 1 none" in line[0] and "->" in line[0]
    items = json.load(open(tmp_path / "map.json"))["items"]
    assert [it["attributes"]["marking"] for it in items] == ["solid", "dashed", "none"]
    assert all("painted_share" in it["attributes"] and "source_line" in it["attributes"] for it in items)


def test_refine_predictions_scores_a_detector_run(tmp_path):
    """The painted drive seen by a detector: four frames whose BEV pixels are lines A and B moved 0.1 m
    to the left.  No GT anywhere: the clusters' markings and the paint's offset come from the cloud.
    A cluster may run against the lane's direction, so only the offset's size is fixed."""
    import json
    import subprocess
    import sys
    import _fuse_oracle as FO
    from pointnet_refine_amd import link as LK
    from pointnet_refine_amd.pcd import write_pcd_host
    poses, cloud, lines = C.painted_drive()
    drive = tmp_path / "drive"
    (drive / "pose").mkdir(parents=True)
    write_pcd_host(str(drive / "merged.pcd"), cloud.astype(np.float64))
    results = {}
    for k, pose in enumerate(poses):
        ts = 1000 + k
        json.dump({"ts": str(ts), "x": pose[0], "y": pose[1], "z": pose[2], "qx": pose[3], "qy": pose[4], "qz": pose[5],
                   "qw": pose[6]}, open(drive / "pose" / f"{ts}.json", "w"))
        inst = []
        for l in lines[:2]:
            u = np.linspace(0.0, 1.0, 601)[:, None]
            lane = l[0] + u * (l[-1] - l[0]) + [0.0, 0.1, 0.0]
            ego = FO.to_ego(lane, pose)
            ego = ego[np.abs(ego[:, 0]) <= 24.0][::20]
            inst.append({"data": np.stack([(25.0 - ego[:, 1]) / 0.05, (25.0 - ego[:, 0]) / 0.05], 1).tolist(), "score": 0.9})
        results[f"cam/{ts}.jpg"] = {"pred_instances": inst}
    json.dump(results, open(tmp_path / "results.json", "w"))
    model = _zero_head_model()
    res = LK.refine_predictions(model, str(drive), str(tmp_path / "results.json"), support=True, intensity_floor=20.0)
    sup = res["support"]
    assert set(sup) == {"fused", "attributes"} and len(res["fused"]) == len(sup["attributes"]) == 2
    by_y = np.argsort([float(np.concatenate(f)[:, 1].mean()) for f in res["fused"]])
    print("markings:", [a["marking"] for a in sup["attributes"]], "offset_w_mean per cluster:",
          [p["offset_w_mean"] for p in sup["fused"]["per_line"]])
    assert [sup["attributes"][c]["marking"] for c in by_y] == ["solid", "dashed"]
    assert all(abs(abs(p["offset_w_mean"]) - 0.1) <= 0.02 for p in sup["fused"]["per_line"])
    plain = LK.refine_predictions(model, str(drive), str(tmp_path / "results.json"))
    assert "support" not in plain and set(res) == set(plain) | {"support"}
    ckpt = tmp_path / "model.pth"
    torch.save(model.cpu().state_dict(), ckpt)
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out = subprocess.run([sys.executable, os.path.join(root, "examples", "refine_predictions.py"), str(drive),
                          str(tmp_path / "results.json"), "--checkpoint", str(ckpt), "--out", str(tmp_path / "map.json"),
                          "--support", "--intensity-floor", "20"], capture_output=True, text=True, timeout=300)
    print(out.stdout[-2000:], out.stderr[-2000:])
    assert out.returncode == 0 and "MAP SUPPORT" in out.stdout and "1 solid, 1 dashed" in out.stdout
    items = json.load(open(tmp_path / "map.json"))["items"]
    assert sorted(it["attributes"]["marking"] for it in items) == ["dashed", "solid"]
