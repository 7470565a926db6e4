"""The per-slice and the batched mode of refine_drive / refine_predictions on a drive small enough
to hit every case the slice refinement branches on: a slice with candidates and points, a slice with
points and no candidate, a slice with candidates and no point, and a tube below min_tube_points.

Public functions only, and the zero-head procedural model of test_refine_batched_gpu.py: offsets of
exactly 0, so the two modes are compared byte for byte.  The integer reports below are recorded
results: they were written down from a run of the code as it stood before the two loops were
folded into fuse.refine_slices, and hold for both modes.

4 poses 25 m apart.  refine_drive cuts 20 m slices at a 20 m stride from them (x in [-10,10],
[15,35], [40,60], [65,85]); a detector frame is 50 m long, one per pose.  The cloud ends at x = 48,
before the last pose, and has no point under the lane at y = -1.7 beyond x = 2."""
import functools
import json

import numpy as np
import pytest

import _fuse_oracle as O
from test_refine_batched_gpu import _gpu_model
from pointnet_refine_amd import fuse as F
from pointnet_refine_amd import link as LK

pytestmark = pytest.mark.gpu
M = 32
LANE_Y = (-1.7, 1.9)
DRIVE_KW = dict(segment_len=20.0, stride=20.0)

DRIVE_REPORT = {'slices': 4, 'pieces': 1, 'pieces_sparse': 2, 'nodes': 136, 'nodes_used': 40, 'fused_polylines': 1}
PREDICTIONS_REPORT = {'slices': 4, 'pieces': 3, 'pieces_sparse': 3, 'nodes': 140, 'nodes_used': 140, 'fused_polylines': 1,
                      'candidates': 1, 'edges': 1, 'clusters': 2, 'clusters_kept': 1, 'pieces_unlinked': 1}
PREDICTIONS_LIFT_ALIGN_REPORT = {'slices': 4, 'pieces': 4, 'pieces_sparse': 2, 'nodes': 280, 'nodes_used': 280, 'fused_polylines': 2,
                                 'candidates': 2, 'edges': 2, 'clusters': 2, 'clusters_kept': 2, 'pieces_unlinked': 0,
                                 'lift_lines': 6, 'lift_lines_lifted': 4, 'lift_lines_unlifted': 2, 'lift_stations': 277,
                                 'lift_stations_without_ground': 180, 'align_frames': 4, 'align_frames_aligned': 2,
                                 'align_frames_unaligned': 2, 'align_candidates': 8317}


@functools.lru_cache(maxsize=None)
def _poses():
    poses = np.zeros((4, 7))
    for k in range(4):
        poses[k, :3] = [25.0 * k, 0.1 * k, 0.0]
        poses[k, 3:] = O.quat_yaw_pitch(0.01 * (k - 1.5), 0.0)
    return poses


@functools.lru_cache(maxsize=None)
def _cloud():
    """About 8 k ground points over x in [-12, 48], none under the first lane beyond x = 2."""
    rng = np.random.default_rng(23)
    n = 9000
    c = np.stack([rng.uniform(-12.0, 48.0, n), rng.uniform(-4.0, 4.0, n), rng.normal(0.0, 0.02, n),
                  rng.uniform(0.0, 60.0, n)], 1).astype(np.float32)
    return c[~((c[:, 0] > 2.0) & (np.abs(c[:, 1] - LANE_Y[0]) < 0.7))]


def _lines():
    """The short line lies past the cloud; the other one ends before the third slice, which so has
    points and no candidate, and loses its tube in the second."""
    return [np.array([[66.0, 1.9, 0.0], [75.0, 1.8, 0.0], [84.0, 1.9, 0.0]]),
            np.array([[-12.0, -1.7, 0.0], [10.0, -1.7, 0.0], [37.0, -1.7, 0.0]])]


def _same(a, b):
    return type(a) is type(b) and (np.array_equal(a, b) and a.dtype == b.dtype if isinstance(a, np.ndarray) else a == b)


def _ints(report):
    return {k: int(v) for k, v in report.items() if isinstance(v, (int, np.integer))}


def _assert_modes_agree(a, b, index_key):
    assert a["report"].keys() == b["report"].keys()
    for k in a["report"]:
        assert _same(a["report"][k], b["report"][k]), k
    for k in (index_key, "piece_slice"):
        assert a[k].dtype == b[k].dtype == np.int64 and np.array_equal(a[k], b[k]), k
    assert a["pieces"].dtype == b["pieces"].dtype == np.float64 and a["pieces"].shape == b["pieces"].shape
    assert a["pieces"].tobytes() == b["pieces"].tobytes()
    assert len(a["fused"]) == len(b["fused"])
    for fa, fb in zip(a["fused"], b["fused"]):
        assert len(fa) == len(fb) and all(x.shape == y.shape and x.tobytes() == y.tobytes() for x, y in zip(fa, fb))
    for k in ("X", "W", "C", "spread", "offsets"):
        assert a["nodes"][k].tobytes() == b["nodes"][k].tobytes(), k


def _slice_cases(cands_per_slice, res, poses):
    """Which of the four cases each slice is, from public calls: the slice's point count and the
    candidates it was given, and the pieces that came back."""
    from pointnet_refine_amd import drive as D
    _, offsets, _ = D.slice_cloud(_cloud(), poses, res["segment_len"], 60.0)
    n_pts = np.diff(offsets.cpu().numpy())
    n_cand = np.array(cands_per_slice)
    got = np.bincount(res["piece_slice"], minlength=len(n_cand))
    return {"both": int(((n_cand > 0) & (n_pts > 0)).sum()), "no_candidate": int(((n_cand == 0) & (n_pts > 0)).sum()),
            "no_point": int(((n_cand > 0) & (n_pts == 0)).sum()),
            "short_tube": int((n_cand - got)[(n_cand > 0) & (n_pts > 0)].sum()),
            "sparse_expected": int(n_cand[n_pts == 0].sum() + (n_cand - got)[n_pts > 0].sum())}


# ------------------------------------------------------------------ refine_drive
@functools.lru_cache(maxsize=None)
def _drive(batched):
    return F.refine_drive(_gpu_model(True), _cloud(), _poses(), _lines(), batched=batched, **DRIVE_KW)


def test_refine_drive_modes_agree():
    from pointnet_refine_amd import drive as D
    a, b = _drive(False), _drive(True)
    print("refine_drive report:", a["report"])
    _assert_modes_agree(a, b, "piece_line")
    assert a["pose_index"] == [0, 1, 2, 3]
    clipped = D.clip_lines(_lines(), a["poses"], DRIVE_KW["segment_len"])
    cases = _slice_cases([len(k) for k in clipped], dict(a, segment_len=DRIVE_KW["segment_len"]), a["poses"])
    print("refine_drive cases:", cases)
    assert cases["both"] >= 1 and cases["no_candidate"] >= 1 and cases["no_point"] >= 1 and cases["short_tube"] >= 1
    assert a["report"]["pieces_sparse"] == cases["sparse_expected"] and a["report"]["pieces"] >= 1
    assert a["report"]["fused_polylines"] >= 1
    # every piece is the clipped candidate it came from, moved by an offset of exactly 0: its line
    # is the line whose clip starts where the piece starts
    for p, l, s in zip(a["pieces"], a["piece_line"], a["piece_slice"]):
        start = dict(clipped[s])[int(l)][0]
        assert np.abs(p[0] - start).max() < 1e-3
    assert _ints(a["report"]) == DRIVE_REPORT


# ------------------------------------------------------------------ refine_predictions
def _write_detector_drive(root, gap=0):
    """The poses as pose files and a detector JSON: both lanes as every frame's BEV sees them, the
    third frame without any instance.  gap shifts the result timestamps away from the poses'."""
    from pointnet_refine_amd.pcd import write_pcd_host
    drive = root / "drive"
    (drive / "pose").mkdir(parents=True)
    write_pcd_host(str(drive / "merged.pcd"), _cloud().astype(np.float64))
    results = {}
    for k, pose in enumerate(_poses()):
        ts = 1000 + k
        json.dump({"ts": str(ts), "x": pose[0], "y": pose[1], "z": pose[2], "qx": pose[3], "qy": pose[4], "qz": pose[5],
                   "qw": pose[6]}, open(drive / "pose" / f"{ts}.json", "w"))
        inst = []
        for y in LANE_Y if k != 2 else ():
            lane = np.stack([np.linspace(-40.0, 120.0, 641), np.full(641, y), np.zeros(641)], 1)
            ego = O.to_ego(lane, pose)
            ego = ego[np.abs(ego[:, 0]) <= 24.0][::20]
            inst.append({"data": np.stack([(25.0 - ego[:, 1]) / 0.05, (25.0 - ego[:, 0]) / 0.05], 1).tolist(), "score": 0.9})
        results[f"cam/{ts + gap}.jpg"] = {"pred_instances": inst}
    json.dump(results, open(root / "results.json", "w"))
    return str(drive), str(root / "results.json")


def test_refine_predictions_modes_agree(tmp_path):
    drive, results = _write_detector_drive(tmp_path)
    a, b = (LK.refine_predictions(_gpu_model(True), drive, results, batched=m) for m in (False, True))
    print("refine_predictions report:", a["report"])
    _assert_modes_agree(a, b, "piece_frame")
    assert np.array_equal(a["piece_frame"], a["piece_slice"])
    cases = _slice_cases([2, 2, 0, 2], dict(a, segment_len=50.0), a["poses"])
    print("refine_predictions cases:", cases)
    assert cases["both"] >= 1 and cases["no_candidate"] >= 1 and cases["no_point"] >= 1 and cases["short_tube"] >= 1
    assert a["report"]["pieces_sparse"] == cases["sparse_expected"] and a["report"]["pieces"] >= 2
    assert a["report"]["fused_polylines"] >= 1
    assert _ints(a["report"]) == PREDICTIONS_REPORT


def test_refine_predictions_lift_align_modes_agree(tmp_path):
    drive, results = _write_detector_drive(tmp_path)
    a, b = (LK.refine_predictions(_gpu_model(True), drive, results, batched=m, lift=True, align=True, support=True)
            for m in (False, True))
    print("refine_predictions lift align report:", a["report"])
    _assert_modes_agree(a, b, "piece_frame")
    assert "lift_lines" in a["report"] and "align_frames" in a["report"]
    sa, sb = a["support"]["fused"], b["support"]["fused"]
    assert sa["nodes"] == sb["nodes"] > 0 and sa["support"]["acc"].tobytes() == sb["support"]["acc"].tobytes()
    assert _ints(a["report"]) == PREDICTIONS_LIFT_ALIGN_REPORT


# ------------------------------------------------------------------ nothing to refine
def _assert_empty(res, index_key):
    assert res["pieces"].shape == (0, M, 3) and res["pieces"].dtype == np.float64
    for k in (index_key, "piece_slice"):
        assert res[k].shape == (0,) and res[k].dtype == np.int64, k
    assert res["report"]["pieces"] == 0 and res["report"]["pieces_sparse"] == 0 and res["report"]["nodes_used"] == 0
    assert all(f == [] for f in res["fused"])


@pytest.mark.parametrize("batched", [False, True])
def test_nothing_to_refine_keeps_shapes_and_dtypes(tmp_path, batched):
    model = _gpu_model(True)
    res = F.refine_drive(model, _cloud(), _poses(), [], batched=batched, **DRIVE_KW)             # no lines
    _assert_empty(res, "piece_line")
    assert res["report"]["slices"] == 4 and res["fused"] == []
    res = F.refine_drive(model, _cloud(), _poses()[:1], _lines(), batched=batched, **DRIVE_KW)   # no slice
    _assert_empty(res, "piece_line")
    assert res["report"]["slices"] == 0 and res["poses"].shape == (0, 7) and len(res["fused"]) == 2
    drive, results = _write_detector_drive(tmp_path, gap=10 ** 12)                                 # no frame finds a pose
    res = LK.refine_predictions(model, drive, results, batched=batched)
    _assert_empty(res, "piece_frame")
    assert res["report"]["slices"] == 0 and res["poses"].shape == (0, 7) and res["fused"] == []
