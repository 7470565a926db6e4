"""Drive slicer on the GPU: the HIP kernels of csrc/prh_drive.hpp against the reference's outputs
in the g11 fixture and against the numpy restatement in test_drive_cpu.py (same tolerances: local
coordinates, clipped vertices and noisy lines within 1e-9 m; membership, order, counts and keep
decisions exact)."""
import os

import numpy as np
import pytest
import torch

import test_drive_cpu as R

pytestmark = pytest.mark.gpu
TOL = R.TOL


def _drive():
    from pointnet_refine_amd import drive
    return drive


def _synthetic_drive(n_points, n_poses, seed=3, origin=(4.0e5, 5.0e6, 20.0)):
    rng = np.random.default_rng(seed)
    length = 25.0 * (n_poses + 1)
    px = origin[0] + 25.0 * np.arange(1, n_poses + 1) + rng.uniform(-2, 2, n_poses)
    py = origin[1] + 8.0 * np.sin(px / 60.0)
    pz = origin[2] + rng.uniform(-0.2, 0.2, n_poses)
    yaw = rng.uniform(-np.pi, np.pi, n_poses)
    pitch, roll = rng.uniform(-0.05, 0.05, n_poses), rng.uniform(-0.05, 0.05, n_poses)
    cy, sy, cp, sp, cr, sr = np.cos(yaw / 2), np.sin(yaw / 2), np.cos(pitch / 2), np.sin(pitch / 2), np.cos(roll / 2), np.sin(roll / 2)
    q = np.stack([sr * cp * cy - cr * sp * sy, cr * sp * cy + sr * cp * sy, cr * cp * sy - sr * sp * cy,
                  cr * cp * cy + sr * sp * sy], 1)
    poses = np.column_stack([px, py, pz, q])
    x = origin[0] + rng.uniform(-40, length + 40, n_points)
    y = origin[1] + rng.uniform(-90, 90, n_points)
    z = origin[2] + rng.uniform(-2, 8, n_points)
    cloud = np.column_stack([x, y, z, rng.uniform(0, 255, n_points)]).astype(np.float32)
    return cloud, poses


def test_slice_cloud_matches_reference(golden_dir):
    D = _drive()
    z = R.load_g11(golden_dir)
    for d in range(2):
        cloud, poses = z[f"d{d}_cloud"], z[f"d{d}_poses"][z[f"d{d}_chosen"]]
        pts, off, idx = D.slice_cloud(cloud, poses)
        assert pts.is_cuda and pts.dtype == torch.float64 and off.dtype == torch.int64 and idx.dtype == torch.int64
        pts, off, idx = pts.cpu().numpy(), off.cpu().numpy(), idx.cpu().numpy()
        assert np.array_equal(off, z[f"d{d}_offsets"])
        assert np.array_equal(idx, z[f"d{d}_source_index"])
        err = np.abs(pts[:, :3] - z[f"d{d}_points"]).max()
        print(f"drive {d}: {len(idx)} points, local xyz max abs err vs reference {err:.3e}")
        assert err < TOL
        assert np.array_equal(pts[:, 3].astype(np.float32).view(np.uint32), cloud[idx, 3].view(np.uint32))
    # radius-boundary points: inside the x-crop by construction, so emitted exactly when inside the disc
    cloud, poses = z["d0_cloud"], z["d0_poses"][z["d0_chosen"]]
    _, off, idx = D.slice_cloud(cloud, poses)
    off, idx = off.cpu().numpy(), idx.cpu().numpy()
    for r, s, want in zip(z["d0_boundary_rows"], z["d0_boundary_slice"], z["d0_boundary_in_radius"]):
        assert (r in idx[off[s]:off[s + 1]]) == bool(want)


def test_slice_cloud_at_size_matches_restatement():
    D = _drive()
    cloud, poses = _synthetic_drive(5_000_000, 44)
    dev_cloud = torch.from_numpy(cloud).cuda()
    pts, off, idx = D.slice_cloud(dev_cloud, poses)
    pts2, off2, idx2 = D.slice_cloud(cloud, poses)
    assert torch.equal(off, off2) and torch.equal(idx, idx2)
    assert torch.equal(pts.view(torch.int64), pts2.view(torch.int64))             # bitwise, run to run
    pts, off, idx = pts.cpu().numpy(), off.cpu().numpy(), idx.cpu().numpy()
    rp, roff, ridx, margins = R.slice_ref(cloud, poses, return_margin=True)
    n_close = 0
    for s in range(len(poses)):
        rows, m = margins[s]
        close = rows[m < 1e-6]                       # undecidable at fp64 rounding: left out of the comparison
        n_close += len(close)
        a, b = idx[off[s]:off[s + 1]], ridx[roff[s]:roff[s + 1]]
        ka, kb = ~np.isin(a, close), ~np.isin(b, close)
        assert np.array_equal(a[ka], b[kb]), f"slice {s}: membership or order differs"
        pa, pb = pts[off[s]:off[s + 1]][ka], rp[roff[s]:roff[s + 1]][kb]
        assert np.abs(pa[:, :3] - pb[:, :3]).max() < TOL
        assert np.array_equal(pa[:, 3], pb[:, 3])
    print(f"at size: {len(cloud)} points, {len(poses)} slices, {len(idx)} emitted, {n_close} within 1e-6 m of a plane")
    assert len(idx) > 1_000_000
    assert n_close < 1e-5 * len(idx)


def test_slice_cloud_empty_inputs():
    D = _drive()
    pose = np.array([[0, 0, 0, 0, 0, 0, 1.0]])
    pts, off, idx = D.slice_cloud(np.zeros((0, 4), np.float32), pose)
    assert pts.shape == (0, 4) and off.tolist() == [0, 0] and idx.shape == (0,)
    cloud = np.random.default_rng(0).uniform(-20, 20, (1000, 4)).astype(np.float32)
    pts, off, idx = D.slice_cloud(cloud, np.zeros((0, 7)))
    assert pts.shape == (0, 4) and off.tolist() == [0] and idx.shape == (0,)
    far = np.array([[0, 0, 0, 0, 0, 0, 1.0], [5000.0, 0, 0, 0, 0, 0, 1.0], [3.0, 0, 0, 0, 0, 0, 1.0]])
    pts, off, idx = D.slice_cloud(cloud, far)
    off = off.tolist()
    assert off[1] == 1000 and off[2] == 1000 and off[3] == 2000                 # the pose nothing is near: empty
    assert idx[:1000].tolist() == list(range(1000))
    torch.cuda.synchronize()


def test_clip_lines_matches_reference(golden_dir):
    D = _drive()
    z = R.load_g11(golden_dir)
    lines = R.split(z["clip_line_verts"], z["clip_line_len"])
    per_slice, cnt = D.clip_lines(lines, z["clip_poses"], return_counts=True)
    assert np.array_equal(cnt, z["clip_counts"])
    ref = R.split(z["clip_out_verts"], z["clip_counts"].reshape(-1))
    n_l, worst = len(lines), 0.0
    for s, kept in enumerate(per_slice):
        assert [l for l, _ in kept] == np.flatnonzero(z["clip_kept"][s]).tolist()
        for l, v in kept:
            worst = max(worst, np.abs(v - ref[s * n_l + l]).max())
    print(f"clip vs reference: {cnt.size} pairs, max abs err {worst:.3e}")
    assert worst < TOL


def test_clip_lines_generated_pairs_match_restatement():
    D = _drive()
    _, poses = _synthetic_drive(10, 40, seed=8)
    rng = np.random.default_rng(9)
    lines = []
    for k in range(100):
        n = int(rng.integers(0, 60))
        x = poses[0, 0] + rng.uniform(-50, 1100) + np.cumsum(rng.uniform(-1, 4, n)) * (1 if k % 3 else -1)
        y = poses[0, 1] + rng.uniform(-20, 20) + np.cumsum(rng.normal(0, 0.5, n))
        line = np.column_stack([x, y, poses[0, 2] + rng.normal(0, 0.1, n)])
        if n > 4 and k % 5 == 0:
            line[3] = line[2]                                                      # a duplicate vertex
        lines.append(line)
    per_slice, cnt = D.clip_lines(lines, poses, return_counts=True)
    rcnt, rout = R.clip_lines_ref(lines, poses)
    assert cnt.size >= 4000 and np.array_equal(cnt, rcnt)
    assert (rcnt > 1).sum() > 50
    for s, kept in enumerate(per_slice):
        assert [l for l, _ in kept] == np.flatnonzero(rcnt[s] > 1).tolist()
        for l, v in kept:
            assert np.abs(v - rout[s][l]).max() < TOL
    assert D.clip_lines([], poses) == [[] for _ in poses] and D.clip_lines(lines, np.zeros((0, 7))) == []


def test_apply_noise_matches_reference(golden_dir):
    D = _drive()
    z = R.load_g11(golden_dir)
    lines = R.split(z["noise_line_verts"], z["noise_line_len"])
    a = 0
    for l, line in enumerate(lines):
        for k in range(len(z["noise_scales"])):
            n = len(line)
            got = D.apply_noise(line, z["noise_yaw"][l, k], z["noise_shift"][l, k], z["noise_jitter"][a:a + n])
            assert np.abs(got - z["noise_out"][a:a + n]).max() < TOL
            a += n


def test_noisy_candidates_arithmetic_bounds_and_moments():
    D = _drive()
    rng = np.random.default_rng(21)
    scales = (0.1, 0.25, 0.4)
    n_lines, n_v = 70_000, 3
    base = rng.uniform(-25, 25, (n_lines, 1, 3)) * [1, 0.3, 0.02]
    lines = list(base + np.cumsum(rng.uniform(0.5, 3, (n_lines, n_v, 3)) * [1, 0.1, 0.01], axis=1))
    lines[0] = np.column_stack([np.linspace(-20, 20, 50), np.sin(np.linspace(0, 3, 50)), np.zeros(50)])
    cands, draws = D.noisy_candidates(lines, scales, seed=5, return_draws=True)
    yaw, shift = draws["yaw"], draws["shift"]
    for l in list(range(0, 200)) + [n_lines - 1]:
        for k in range(3):
            want = R.apply_noise_ref(lines[l], yaw[l, k], shift[l, k], draws["jitter"][l][k])
            assert np.abs(cands[l][k] - want).max() < TOL
    s = np.array(scales)
    assert (np.abs(yaw) <= (5.0 * s) * (np.pi / 180.0)).all()
    assert (np.abs(shift[:, :, 0]) <= s).all() and (np.abs(shift[:, :, 1]) <= s).all()
    assert (np.abs(shift[:, :, 2]) <= 0.1).all()
    # >= 2e5 draws of each kind; 1 % is six standard errors or more (0.16 % for a standard deviation,
    # 0.13 % of the half-range for a uniform mean at that count)
    unit = {"yaw": yaw / ((5.0 * s) * (np.pi / 180.0)), "dx": shift[:, :, 0] / s, "dy": shift[:, :, 1] / s,
            "dz": shift[:, :, 2] / 0.1}
    for name, u in unit.items():
        assert u.size >= 200_000
        print(f"{name}: mean / half-range {u.mean():+.5f}, std {u.std():.5f} (uniform: 0.57735)")
        assert abs(u.mean()) < 0.01
        assert abs(u.std() - 1 / np.sqrt(3)) < 0.01
    jit = np.concatenate([j.reshape(-1, 3) for j in draws["jitter"]])
    assert len(jit) >= 200_000
    for c, sigma in enumerate((0.05, 0.05, 0.025)):
        sd = jit[:, c].std()
        print(f"jitter {c}: std {sd:.6f} (want {sigma}), mean {jit[:, c].mean():+.2e}")
        assert abs(sd - sigma) < 0.01 * sigma
        assert abs(jit[:, c].mean()) < 0.01 * sigma
    again = D.noisy_candidates(lines[:50], scales, seed=5)
    assert all(np.array_equal(again[l][k], cands[l][k]) for l in range(50) for k in range(3))    # bitwise
    other = D.noisy_candidates(lines[:50], scales, seed=6)
    assert not np.array_equal(other[1][0], cands[1][0])
    assert not np.array_equal(draws["jitter"][1][0], draws["jitter"][2][0])                      # line
    assert yaw[1, 0] / s[0] != yaw[1, 1] / s[1] and not np.array_equal(draws["jitter"][1][0], draws["jitter"][1][1])
    assert D.noisy_candidates([], scales) == []


def _write_drive(root, with_lanes=True):
    import json
    cloud, poses = _synthetic_drive(60_000, 8, seed=12, origin=(1000.0, 2000.0, 5.0))
    cloud[:, 1] = 2000.0 + np.random.default_rng(1).uniform(-15, 15, len(cloud))
    os.makedirs(os.path.join(root, "pose"))
    for i, p in enumerate(poses):
        with open(os.path.join(root, "pose", f"{i:06d}.json"), "w") as f:
            json.dump(dict(zip(("x", "y", "z", "qx", "qy", "qz", "qw"), map(float, p))), f)
    with open(os.path.join(root, "merged.pcd"), "wb") as f:
        f.write((f"VERSION 0.7\nFIELDS x y z intensity\nSIZE 4 4 4 4\nTYPE F F F F\nCOUNT 1 1 1 1\nWIDTH {len(cloud)}\n"
                 f"HEIGHT 1\nVIEWPOINT 0 0 0 1 0 0 0\nPOINTS {len(cloud)}\nDATA binary\n").encode())
        f.write(cloud.astype("<f4").tobytes())
    xs = np.linspace(poses[0, 0] - 30, poses[-1, 0] + 30, 80)
    lanes = [np.column_stack([xs, 2000.0 + 3.5 * k + 0.5 * np.sin(xs / 20), np.full_like(xs, 5.0)]) for k in range(-1, 2)]
    gt = os.path.join(root, "gt.json")
    with open(gt, "w") as f:
        json.dump({"items": [{"category": "lane", "attributes": {"id": k},
                              "position": [dict(zip("xyz", map(float, v))) for v in l]} for k, l in enumerate(lanes)]}, f)
    return gt, cloud, poses


def test_drive_to_stream_end_to_end(tmp_path):
    D = _drive()
    from pointnet_refine_amd.context import resample_polyline
    from pointnet_refine_amd.io import SceneSampleStream, load_pcd_data, load_scene_items
    drive_dir, out_dir, out2 = str(tmp_path / "drive"), str(tmp_path / "scenes"), str(tmp_path / "stored")
    os.makedirs(drive_dir)
    gt, cloud, poses = _write_drive(drive_dir)
    res = D.slice_drive(drive_dir, gt, out_dir, verbose=False)
    assert len(res["written"]) >= 3 and res["pose_index"] == D.plan_slices(poses)
    name = res["written"][0]
    s = res["names"].index(name)
    off = res["offsets"].cpu().numpy()
    back = load_pcd_data(os.path.join(out_dir, name + ".pcd"))
    assert len(back) == off[s + 1] - off[s]
    assert np.abs(back[:, :3] - res["points"][off[s]:off[s + 1], :3].cpu().numpy()).max() < 1e-4
    items = load_scene_items(os.path.join(out_dir, name + ".json"))
    assert len(items) == len(res["items"][s]) > 0 and all(it["noisy_candidates"] == [] for it in items)

    assert len(SceneSampleStream(out_dir, num_context_points=256, batch_size=8)) == 0       # GT only
    scales = (0.1, 0.25, 0.4)
    st = SceneSampleStream(out_dir, num_context_points=256, batch_size=8, augment=scales, seed=3)
    n_items = sum(len(res["items"][res["names"].index(n)]) for n in res["written"])
    assert len(st) == 3 * n_items

    def epoch(stream, e):
        stream.set_epoch(e)
        return list(stream)

    e0, e0b, e1 = epoch(st, 0), epoch(st, 0), epoch(st, 1)
    assert sum(b["context"].shape[0] for b in e0) == len(st)
    for b in e0:
        n = b["context"].shape[0]
        assert set(b) == {"context", "noisy_line", "target_offset", "points_in_tube"}
        assert b["context"].shape == (n, 256, 4) and b["noisy_line"].shape == (n, 32, 3)
        assert b["target_offset"].shape == (n, 32, 3) and b["context"].is_cuda
    for a, b in zip(e0, e0b):
        assert all(torch.equal(a[k], b[k]) for k in a)
    assert not torch.equal(torch.cat([b["noisy_line"] for b in e0]).sort(0).values,
                           torch.cat([b["noisy_line"] for b in e1]).sort(0).values)
    # target_offset + noisy_line = the resampled GT, centred on the noisy line's mean: per scene
    one = SceneSampleStream(out_dir, num_context_points=256, batch_size=None, augment=scales, seed=3, shuffle=False)
    for batch in one:
        its = load_scene_items(batch["scene"].replace(".pcd", ".json"))
        gts = np.stack([resample_polyline(it["position"], 32) for it in its for _ in scales])
        total = (batch["target_offset"] + batch["noisy_line"]).double().cpu().numpy()
        centred = gts - gts.mean(axis=1, keepdims=True)
        shift = total - centred                      # = GT mean - noisy mean: one constant per sample
        assert np.abs(shift - shift.mean(axis=1, keepdims=True)).max() < 1e-3
        assert np.abs(shift.mean(axis=1)).max() < 0.6          # |shift| <= 0.4 + jitter

    # stored candidates: augment=None is the stream as it was
    D.slice_drive(drive_dir, gt, out2, candidates=True, verbose=False)
    a = list(SceneSampleStream(out2, num_context_points=256, batch_size=8, seed=3))
    b = list(SceneSampleStream(out2, num_context_points=256, batch_size=8, seed=3, augment=None))
    assert len(a) == len(b) > 0 and sum(x["context"].shape[0] for x in a) == 3 * n_items
    for x, y in zip(a, b):
        assert all(torch.equal(x[k], y[k]) for k in x)
