"""Prediction scenes on the GPU (csrc/prh_match.hpp through pointnet_refine_amd.predictions): the
frame clip, the cost matrices and the batched assignment against the g12 fixture the reference's
tool produced and against the numpy restatement of test_predictions_cpu.py.  Tolerances as there:
1e-9 m on vertices and costs, decisions exact.  The assignment at size is checked without a
reference solver, by its optimality certificate, and exactly against the restatement wherever the
optimum is unique by >= 1e-6."""
import json
import os

import numpy as np
import pytest
import torch

import test_predictions_cpu as R

pytestmark = pytest.mark.gpu
TOL = R.TOL


def _pr():
    from pointnet_refine_amd import predictions
    return predictions


def _offsets(counts):
    return np.concatenate(([0], np.cumsum(counts))).astype(np.int64)


def _flatten(frames):
    preds = [l for p, _ in frames for l in p]
    gts = [l for _, g in frames for l in g]
    return preds, _offsets([len(p) for p, _ in frames]), gts, _offsets([len(g) for _, g in frames])


def test_clip_lines_frames_matches_reference(golden_dir):
    PR = _pr()
    z = R.load_g12(golden_dir)
    lanes = R.split(z["gt_verts"], z["gt_len"])
    per_frame, counts = PR.clip_lines_frames(lanes, z["poses"], return_counts=True)
    assert np.array_equal(counts, z["clip_counts"])
    got = np.concatenate([v for f in range(len(z["poses"])) for l, v in per_frame[f]] or [np.zeros((0, 3))])
    want = R.split(z["clip_verts"], z["clip_counts"][z["clip_counts"] > 0])
    want = np.concatenate([w for w in want if len(w) > 1])
    assert got.shape == want.shape and np.abs(got - want).max() < TOL
    for f in range(len(z["poses"])):
        assert [l for l, _ in per_frame[f]] == np.flatnonzero(z["clip_counts"][f] > 1).tolist()
    # the context lines of the frames the tool wrote
    ctx = R.split(z["ctx_verts"], z["ctx_len"])
    for k, j in enumerate(z["written_pose"]):
        a, b = z["ctx_offsets"][k], z["ctx_offsets"][k + 1]
        assert [l for l, _ in per_frame[j]] == z["ctx_lane"][a:b].tolist()
        for (_, v), w in zip(per_frame[j], ctx[a:b]):
            assert np.abs(v - w).max() < TOL
    assert PR.clip_lines_frames([], z["poses"]) == [[] for _ in z["poses"]]
    assert PR.clip_lines_frames(lanes, np.zeros((0, 7))) == []
    bad = z["poses"][:2].copy()
    bad[1, 3:] *= 1.00001
    with pytest.raises(ValueError, match="pose 1"):
        PR.clip_lines_frames(lanes, bad)


def test_clip_lines_frames_generated_pairs_match_restatement():
    PR = _pr()
    rng = np.random.default_rng(4)
    yaw = rng.uniform(-np.pi, np.pi, 24)
    poses = np.column_stack([4.0e5 + rng.uniform(0, 200, 24), 5.0e6 + rng.uniform(0, 200, 24), rng.uniform(0, 5, 24),
                             np.zeros(24), np.zeros(24), np.sin(yaw / 2), np.cos(yaw / 2)])
    lines = []
    for _ in range(150):
        n = int(rng.integers(1, 40))
        a = np.array([4.0e5 + rng.uniform(0, 200), 5.0e6 + rng.uniform(0, 200), 0.0])
        lines.append(a + np.cumsum(rng.normal(0, 6, (n, 3)) * [1, 1, 0.01], axis=0))
    lines.append(np.zeros((0, 3)))
    per_frame, counts = PR.clip_lines_frames(lines, poses, return_counts=True)
    want_counts, want = R.clip_lines_frames_ref(lines, poses)
    assert np.array_equal(counts, want_counts) and (counts > 1).sum() > 100 and (counts == 1).sum() > 0
    for f in range(len(poses)):
        for l, v in per_frame[f]:
            assert np.abs(v - want[f][l]).max() < TOL


def test_each_clip_entry_point_runs_its_own_rule():
    """drive.clip_lines and clip_lines_frames share one driver on each side of the C ABI; two lines
    on which the two rules differ show that each entry point still launches its own kernel.  One
    identity pose (the frame transform is exact), segment_len 50.  Line A ends on the slab's two
    faces: the slicer keeps both end points (x_min <= x <= x_max), this tool's gate finds no vertex
    strictly inside and drops it.  Line B crosses both faces and is cut at +-25 by either rule.
    Every value is exact in fp64, so counts and vertices are compared with ==."""
    from pointnet_refine_amd import drive
    PR = _pr()
    pose = np.array([[0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 1.0]])
    a = np.array([(-25.0, 0.0, 0.0), (25.0, 0.0, 0.0)])
    b = np.array([(-30.0, 1.0, 0.0), (0.0, 1.0, 0.0), (30.0, 1.0, 0.0)])
    b_cut = np.array([(-25.0, 1.0, 0.0), (0.0, 1.0, 0.0), (25.0, 1.0, 0.0)])
    want = {drive.clip_lines: ([2, 3], [(0, a), (1, b_cut)], R.RD.clip_lines_ref),
            PR.clip_lines_frames: ([0, 3], [(1, b_cut)], R.clip_lines_frames_ref)}
    for fn, (counts, kept, restatement) in want.items():
        ref_counts, ref = restatement([a, b], pose)                 # the hand-derived table, on the CPU
        assert ref_counts.tolist() == [counts] and all(np.array_equal(ref[0][l], v) for l, v in kept)
        per_pose, got_counts = fn([a, b], pose, segment_len=50.0, return_counts=True)
        assert got_counts.tolist() == [counts]
        assert len(per_pose) == 1 and [l for l, _ in per_pose[0]] == [l for l, _ in kept]
        for (_, v), (_, w) in zip(per_pose[0], kept):
            assert v.dtype == np.float64 and np.array_equal(v, w)
        per_pose, got_counts = fn([], pose, return_counts=True)
        assert per_pose == [[]] and got_counts.shape == (1, 0)
        per_pose, got_counts = fn([a, b], np.zeros((0, 7)), return_counts=True)
        assert per_pose == [] and got_counts.shape == (0, 2)


def test_costs_and_matches_on_reference_frames(golden_dir):
    PR = _pr()
    z = R.load_g12(golden_dir)
    frames = R._frames_of(z)
    res = PR.match_predictions([f[0] for f in frames], [f[1] for f in frames])
    preds, p_off, gts, g_off = _flatten([(f[0], f[1]) for f in frames])
    costs, c_off, shapes = PR.line_costs(preds, p_off, gts, g_off)
    match, total, u, v = PR.assign(costs, c_off, shapes, return_duals=True)
    assert np.array_equal(shapes, z["cost_shapes"])
    costs = costs.cpu().numpy()
    for k, (ts, (pl, gl, want, cost)) in enumerate(zip(z["written_ts"], frames)):
        got = costs[c_off[k]:c_off[k + 1]].reshape(shapes[k])
        assert np.array_equal(res[k][1], got)
        if cost.size:
            assert np.abs(got - cost).max() < TOL
        m = match[p_off[k]:p_off[k + 1]]
        R.check_certificate(got, m, total[k], u[p_off[k]:p_off[k + 1]], v[g_off[k]:g_off[k + 1]])
        if int(ts) != int(z["tie_ts"]):
            thr = np.where((m >= 0) & (got[np.arange(len(m)), np.maximum(m, 0)] < 15.0), m, -1) if cost.size else m
            assert thr.tolist() == want.tolist() == res[k][0].tolist()
        else:
            assert abs(total[k] - cost[np.arange(len(want)), want].sum()) < TOL


def test_costs_and_assignment_at_size():
    PR = _pr()
    frames = R.random_frames()
    preds, p_off, gts, g_off = _flatten(frames)
    costs_t, c_off, shapes = PR.line_costs(preds, p_off, gts, g_off)
    again, _, _ = PR.line_costs(preds, p_off, gts, g_off)
    assert torch.equal(costs_t, again)                                  # bitwise, run to run
    costs = costs_t.cpu().numpy()
    want = R.costs_ref_threaded(frames)
    worst = max(float(np.abs(costs[c_off[f]:c_off[f + 1]].reshape(shapes[f]) - want[f]).max(initial=0.0))
                for f in range(len(frames)))
    print(f"costs: {len(frames)} frames, {len(preds)} x {len(gts)} lines, {c_off[-1]} entries, worst |diff| {worst:.3e}")
    assert worst < TOL
    match, total, u, v = PR.assign(costs_t, c_off, shapes, return_duals=True)
    m2, t2, u2, v2 = PR.assign(costs_t, c_off, shapes, return_duals=True)
    assert np.array_equal(match, m2) and np.array_equal(total, t2) and np.array_equal(u, u2) and np.array_equal(v, v2)
    left_out = 0
    for f in range(len(frames)):
        cost = costs[c_off[f]:c_off[f + 1]].reshape(shapes[f])
        m = match[p_off[f]:p_off[f + 1]]
        R.check_certificate(cost, m, total[f], u[p_off[f]:p_off[f + 1]], v[g_off[f]:g_off[f + 1]])
        ref, ref_total = R.assign_ref(cost)
        assert abs(total[f] - ref_total) <= 1e-9 * max(1.0, np.abs(cost).max(initial=0.0)) * max(1, min(cost.shape))
        if not np.array_equal(m, ref):                  # only a frame whose optimum is not unique may differ
            assert not R.unique_by(cost), f
            left_out += 1
    print(f"assignment: {left_out} of {len(frames)} frames differ from the restatement (non-unique optimum)")
    assert left_out <= 0.01 * len(frames)
    # the threshold only removes pairs
    thr, _ = PR.assign(costs_t, c_off, shapes, threshold=15.0)
    row_cost = np.concatenate([costs[c_off[f]:c_off[f + 1]].reshape(shapes[f])[np.arange(shapes[f][0]),
                               np.maximum(match[p_off[f]:p_off[f + 1]], 0)] if shapes[f][1] else np.zeros(shapes[f][0])
                               for f in range(len(frames))])
    assert np.array_equal(thr, np.where((match >= 0) & (row_cost < 15.0), match, -1)) and (thr != match).any()


def test_lane_frames_match_their_source():
    PR = _pr()
    lanes = R.lane_frames()
    res = PR.match_predictions([p for p, _, _ in lanes], [g for _, g, _ in lanes])
    for (preds, gts, src), (match, cost) in zip(lanes, res):
        assert np.abs(cost - R.cost_frame_ref(preds, gts)).max(initial=0.0) < TOL
        R.assert_sole_predictions_matched(match, src)
        ref = R.assign_ref(cost)[0]
        assert np.array_equal(match, ref) or not R.unique_by(cost)


def test_empty_inputs_and_bad_costs():
    PR = _pr()
    line = np.array([[0.0, 0, 0], [1.0, 0, 0]])
    costs, c_off, shapes = PR.line_costs([], [0], [], [0])
    assert costs.numel() == 0 and c_off.tolist() == [0] and shapes.shape == (0, 2)
    match, total = PR.assign(costs, c_off, shapes)
    assert match.shape == (0,) and total.shape == (0,)
    assert PR.match_predictions([], []) == []
    # P = 0 and G = 0 frames around a real one
    res = PR.match_predictions([[], [line, line + 1], [line]], [[line], [], [line + [0, 3, 0]]])
    assert res[0][0].shape == (0,) and res[0][1].shape == (0, 1)
    assert res[1][0].tolist() == [-1, -1] and res[1][1].shape == (2, 0)
    assert res[2][0].tolist() == [0] and abs(res[2][1][0, 0] - 3.0) < TOL
    match, total = PR.assign(np.zeros(0), [0, 0, 0], [[3, 0], [0, 2]])
    assert match.tolist() == [-1, -1, -1] and total.tolist() == [0.0, 0.0]
    # a non-finite cost is refused by name, and the kernel returns normally
    good = np.arange(6, dtype=np.float64)
    for bad_value in (np.nan, np.inf, -np.inf):
        bad = np.arange(12, dtype=np.float64)
        bad[7] = bad_value
        with pytest.raises(ValueError, match="frame 1"):
            PR.assign(np.concatenate([good, bad]), [0, 6, 18], [[2, 3], [4, 3]])
    match, total = PR.assign(good, [0, 6], [[2, 3]])                    # the device is fine afterwards
    assert match.tolist() == [0, 1] and total[0] == 4.0
    with pytest.raises(ValueError, match="at most 128"):
        PR.assign(np.zeros(129), [0, 129], [[129, 1]])
    with pytest.raises(ValueError):
        PR.assign(np.zeros(5), [0, 6], [[2, 3]])


def test_predictions_to_scenes_end_to_end(golden_dir, tmp_path):
    PR = _pr()
    from oracle import procedural as P
    from pointnet_refine_amd.io import SceneSampleStream, load_pcd_data, load_scene_items
    from pointnet_refine_amd.metrics import evaluate_scene
    from pointnet_refine_amd.model import LineRefineNet
    z = R.load_g12(golden_dir)
    drive_dir, gt, results = R._write_drive(z, str(tmp_path / "drive"))
    out_dir = str(tmp_path / "scenes")
    res = PR.predictions_to_scenes(drive_dir, gt, results, out_dir, verbose=False)
    # the frames, poses and slices the reference's main() wrote
    assert res["frames"] == z["frame_ts"].tolist() and res["pose_index"] == z["frame_pose"].tolist()
    assert res["written"] == z["written_ts"].tolist()
    assert sorted(os.listdir(out_dir)) == sorted(f"{ts}.{e}" for ts in z["written_ts"] for e in ("json", "pcd"))
    off = res["offsets"].cpu().numpy()
    pts = res["points"].cpu().numpy()
    ctx = R.split(z["ctx_verts"], z["ctx_len"])
    p_off = _offsets(z["frame_n_pred"])
    for k, ts in enumerate(z["written_ts"]):
        n = res["frames"].index(int(ts))
        s = res["slice"][n]
        a, b = z["slice_offsets"][k], z["slice_offsets"][k + 1]
        got = pts[off[s]:off[s + 1]]
        assert len(got) == b - a and np.array_equal(got[:, 3].astype(np.int64), z["slice_source"][a:b])
        assert np.abs(got[:, :3] - z["slice_points"][a:b]).max() < TOL
        back = load_pcd_data(os.path.join(out_dir, f"{ts}.pcd"))
        assert len(back) == b - a and np.abs(back[:, :3] - z["slice_points"][a:b]).max() < 1e-4
        doc = json.load(open(os.path.join(out_dir, f"{ts}.json")))
        assert doc["timestamp"] == str(z["pose_ts"][z["written_pose"][k]]) and doc["result_timestamp"] == str(ts)
        items = load_scene_items(os.path.join(out_dir, f"{ts}.json"))
        want = z["match"][z["match_offsets"][k]:z["match_offsets"][k + 1]]
        lines = ctx[z["ctx_offsets"][k]:z["ctx_offsets"][k + 1]]
        assert len(items) == len(want) == z["frame_n_pred"][n]
        for i, (it, raw) in enumerate(zip(items, doc["items"])):
            assert raw["category"] == "lane_line" and raw["attributes"] == {"score": z["pred_scores"][p_off[n] + i]}
            assert len(it["noisy_candidates"]) == 1 and len(it["context_lines"]) == len(lines)
            assert np.array_equal(it["noisy_candidates"][0], R.split(z["pred_ego"], z["pred_len"])[p_off[n] + i])
            if int(ts) != int(z["tie_ts"]):
                assert res["matches"][n][i] == want[i]
                if want[i] >= 0:
                    assert np.abs(it["position"] - lines[want[i]]).max() < TOL
                else:
                    assert len(it["position"]) == 0
    # the folder feeds the stream and the evaluation
    st = SceneSampleStream(out_dir, num_context_points=256, batch_size=8, augment=(0.25,), seed=1)
    batches = list(st)
    assert len(st) > 0 and sum(b["context"].shape[0] for b in batches) == len(st)
    assert all(b["context"].is_cuda and b["noisy_line"].shape[1:] == (32, 3) for b in batches)
    m = LineRefineNet()
    m.load_state_dict(P.linerefine_state_dict(0))
    m = m.cuda()
    n_rows = 0
    for ts in z["written_ts"]:
        items = load_scene_items(os.path.join(out_dir, f"{ts}.json"))
        ev = evaluate_scene(m, load_pcd_data(os.path.join(out_dir, f"{ts}.pcd")), items, num_context_points=256,
                            crop_radius=0.5)
        matched = np.array([len(items[i]["position"]) > 1 for i in ev["item_index"]])
        assert len(ev["item_index"]) == len(items) and np.array_equal(ev["valid"].astype(bool), matched)
        for key in ("ade_noisy", "ade_refined", "cd_noisy", "cd_refined", "lat_noisy", "lat_refined"):
            assert np.isfinite(ev[key][matched]).all()
        n_rows += int(matched.sum())
    assert n_rows >= 30
