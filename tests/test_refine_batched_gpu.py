"""refine_drive / refine_predictions with batched=True (one io.scene_offsets_ragged call for all
slices) against the per-slice loop they replace, on a synthetic drive and a synthetic detector run
of the kind test_fuse_gpu.py and test_link_gpu.py use, with the default 1024 context points.

The contexts of the two modes are the same bytes (test_context_ragged_gpu.py), so with a zero head
(offsets exactly 0) everything is compared byte for byte.  With the heads left non-zero the modes
differ in which rows share a GEMM call and, on the split-fp16 cores, in the per-tensor scale that
follows from it: each mode's row is within the project's 1e-4 gate of the exact result
(test_oracle_fp64_gpu.py), hence within 2e-4 of the other."""
import functools
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import _fuse_oracle as O
from pointnet_refine_amd import fuse as F
from pointnet_refine_amd import link as LK

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LANE_Y = (-1.7, 1.9)


def _model(zero_head):
    from pointnet_refine_amd.model import LineRefineNet
    from oracle import procedural as P
    m = LineRefineNet()
    m.load_state_dict(P.linerefine_state_dict(0))
    if zero_head:
        with torch.no_grad():
            for branch in m.reg_branches:
                branch[2].weight.zero_()
                branch[2].bias.zero_()
    return m


@functools.lru_cache(maxsize=None)
def _gpu_model(zero_head):
    return _model(zero_head).cuda().eval()


@functools.lru_cache(maxsize=None)
def _synthetic_drive():
    """6 poses 25 m apart near the origin, a ground cloud of 40 k points, two straight lanes and a
    third polyline of 7 vertices that leaves the cloud half way (its later pieces have sparse tubes)."""
    rng = np.random.default_rng(11)
    poses = np.zeros((6, 7))
    for k in range(6):
        poses[k, :3] = [25.0 * k, 0.3 * k, 0.0]
        poses[k, 3:] = O.quat_yaw_pitch(0.04 * (k - 2.5), 0.0)
    n = 40000
    cloud = np.stack([rng.uniform(-8.0, 133.0, n), rng.uniform(-4.0, 4.0, n), rng.normal(0.0, 0.02, n),
                      rng.uniform(0.0, 60.0, n)], 1).astype(np.float32)
    a, b = np.array([-10.3, -1.7, 0.0]), np.array([140.1, -1.3, 0.0])
    x = np.linspace(-9.0, 139.0, 7)
    lines = [np.stack([a, a + 0.473 * (b - a), b]), np.array([[-10.7, 1.9, 0.0], [140.4, 1.6, 0.0]]),
             np.stack([x, 0.2 + np.maximum(0.0, x - 60.0) * 0.4, np.zeros(7)], 1)]
    return poses, cloud, lines


@functools.lru_cache(maxsize=None)
def _drive_result(zero_head, batched, precision=None):
    """refine_drive on the synthetic drive: computed once per mode, shared, never written to."""
    poses, cloud, lines = _synthetic_drive()
    return F.refine_drive(_gpu_model(zero_head), cloud, poses, lines, precision=precision, batched=batched)


def _assert_same_map(a, b, exact):
    assert a["report"] == b["report"]
    for k in ("piece_line", "piece_slice"):
        assert np.array_equal(a[k], b[k]) and a[k].dtype == b[k].dtype, k
    assert a["pieces"].shape == b["pieces"].shape and a["pieces"].dtype == b["pieces"].dtype
    assert [len(f) for f in a["fused"]] == [len(f) for f in b["fused"]]
    if exact:
        assert a["pieces"].tobytes() == b["pieces"].tobytes()
        for fa, fb in zip(a["fused"], b["fused"]):
            assert all(x.shape == y.shape and x.tobytes() == y.tobytes() for x, y in zip(fa, fb))


def test_zero_head_drive_is_byte_identical():
    a, b = _drive_result(True, False), _drive_result(True, True)
    rep = a["report"]
    print(rep)
    assert rep["slices"] >= 4 and rep["pieces"] >= 10 and rep["pieces_sparse"] >= 1      # both outcomes occur
    assert len(set(a["piece_slice"].tolist())) >= 4
    _assert_same_map(a, b, exact=True)


def test_sparse_tubes_are_counted_the_same():
    """The sparse-tube case of test_fuse_gpu.py: the second line has no cloud under it."""
    poses, cloud, lines = _synthetic_drive()
    far = [lines[0], lines[1] + [0.0, 30.0, 0.0]]
    res = [F.refine_drive(_gpu_model(True), cloud, poses, far, batched=b) for b in (False, True)]
    assert res[0]["report"]["pieces_sparse"] == res[0]["report"]["pieces"] > 0
    assert set(res[0]["piece_line"].tolist()) == {0} and res[1]["fused"][1] == []
    _assert_same_map(res[0], res[1], exact=True)
    # a slice without any point: its lines are counted, never sent to the model
    gap = cloud[(cloud[:, 0] < 20.0) | (cloud[:, 0] > 85.0)]
    res = [F.refine_drive(_gpu_model(True), gap, poses, lines[:2], batched=b) for b in (False, True)]
    assert res[0]["report"]["pieces_sparse"] >= 2
    _assert_same_map(res[0], res[1], exact=True)


def test_procedural_model_agrees_within_the_gate():
    a, b = _drive_result(False, False), _drive_result(False, True)
    _assert_same_map(a, b, exact=False)
    moved = float(np.abs(a["pieces"] - _drive_result(True, False)["pieces"]).max())
    worst = float(np.abs(a["pieces"] - b["pieces"]).max())
    print(f"procedural heads, default precision: max |batched - per-slice| = {worst:.3e} m "
          f"(the heads move the pieces by up to {moved:.3e} m)")
    assert moved > 1e-3                                   # the offsets are not zero here
    assert worst <= 2e-4


def test_fp16_precision_stays_within_twice_its_own_error():
    base = _drive_result(False, False)
    loop16, batch16 = _drive_result(False, False, "fp16"), _drive_result(False, True, "fp16")
    _assert_same_map(loop16, batch16, exact=False)
    assert np.array_equal(base["piece_line"], batch16["piece_line"]) and np.array_equal(base["piece_slice"], batch16["piece_slice"])
    e0 = float(np.abs(loop16["pieces"] - base["pieces"]).max())
    e1 = float(np.abs(batch16["pieces"] - base["pieces"]).max())
    print(f"fp16: max |per-slice fp16 - per-slice default| = {e0:.3e} m, max |batched fp16 - per-slice default| = {e1:.3e} m")
    assert e0 > 0.0 and e1 <= 2.0 * e0


# ------------------------------------------------------------------ a detector run
def _write_detector_drive(root):
    """6 poses 25 m apart with a little yaw, a ground cloud of 40 k points that ends before the last
    frame, and a results JSON whose pixels are two straight lanes as each frame's BEV sees them."""
    from pointnet_refine_amd.pcd import write_pcd_host
    rng = np.random.default_rng(7)
    drive = root / "drive"
    (drive / "pose").mkdir(parents=True)
    n = 40000
    cloud = np.column_stack([rng.uniform(-8.0, 120.0, n), rng.uniform(-4.0, 4.0, n), rng.normal(0.0, 0.02, n),
                             rng.uniform(0.0, 60.0, n)])
    write_pcd_host(str(drive / "merged.pcd"), cloud)
    results = {}
    for k in range(6):
        ts = 1000 + k
        pose = np.array([25.0 * (k + 1), 0.3 * k, 0.0, *O.quat_yaw_pitch(0.04 * (k - 1.5), 0.0)])
        json.dump({"ts": str(ts), "x": pose[0], "y": pose[1], "z": pose[2], "qx": pose[3], "qy": pose[4], "qz": pose[5],
                   "qw": pose[6]}, open(drive / "pose" / f"{ts}.json", "w"))
        inst = []
        for y in LANE_Y if k != 2 else LANE_Y[:1]:                    # one frame sees a single lane
            lane = np.stack([np.linspace(-10.0, 190.0, 801), np.full(801, y), np.zeros(801)], 1)
            ego = O.to_ego(lane, pose)
            ego = ego[np.abs(ego[:, 0]) <= 24.0][::20]
            pix = np.stack([(25.0 - ego[:, 1]) / 0.05, (25.0 - ego[:, 0]) / 0.05], 1)
            inst.append({"data": pix.tolist(), "score": 0.9})
        results[f"cam/{ts}.jpg"] = {"pred_instances": inst}
    json.dump(results, open(root / "results.json", "w"))
    return drive


def test_refine_predictions_batched(tmp_path):
    drive = _write_detector_drive(tmp_path)
    ints = None
    for zero_head in (True, False):
        res = [LK.refine_predictions(_gpu_model(zero_head), str(drive), str(tmp_path / "results.json"), batched=b)
               for b in (False, True)]
        print(res[0]["report"])
        assert res[0]["report"] == res[1]["report"] and res[0]["report"]["pieces"] >= 8
        assert res[0]["report"]["pieces_sparse"] >= 1                 # the last frame looks past the cloud
        assert np.array_equal(res[0]["piece_frame"], res[1]["piece_frame"])
        assert np.array_equal(res[0]["piece_slice"], res[1]["piece_slice"])
        if zero_head:
            assert res[0]["pieces"].tobytes() == res[1]["pieces"].tobytes()
            assert len(res[0]["fused"]) == len(res[1]["fused"]) >= 2
            for fa, fb in zip(res[0]["fused"], res[1]["fused"]):
                assert len(fa) == len(fb) and all(x.tobytes() == y.tobytes() for x, y in zip(fa, fb))
            ints = res[0]["report"]
        else:
            assert np.abs(res[0]["pieces"] - res[1]["pieces"]).max() <= 2e-4
    assert ints is not None


def test_example_writes_the_same_map_with_batched(tmp_path):
    from pointnet_refine_amd.pcd import write_pcd_host
    poses, cloud, lines = _synthetic_drive()
    drive = tmp_path / "drive"
    (drive / "pose").mkdir(parents=True)
    for k, p in enumerate(poses):
        json.dump({"ts": str(1000 + k), "x": p[0], "y": p[1], "z": p[2], "qx": p[3], "qy": p[4], "qz": p[5], "qw": p[6]},
                  open(drive / "pose" / f"{1000 + k}.json", "w"))
    write_pcd_host(str(drive / "merged.pcd"), cloud.astype(np.float64))
    F.write_map_json(str(tmp_path / "lines.json"), [[l] for l in lines], categories=["lane"] * len(lines))
    ckpt = tmp_path / "model.pth"
    torch.save(_model(True).state_dict(), ckpt)
    maps = []
    for flags in ([], ["--batched"]):
        out_path = tmp_path / f"map{len(flags)}.json"
        out = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "refine_drive.py"), str(drive),
                              str(tmp_path / "lines.json"), "--checkpoint", str(ckpt), "--out", str(out_path),
                              "--noise", "0.1"] + flags, capture_output=True, text=True, timeout=300)
        print(out.stdout[-1500:], out.stderr[-1500:])
        assert out.returncode == 0
        maps.append(open(out_path, "rb").read())
    assert len(maps[0]) > 1000 and maps[0] == maps[1]
