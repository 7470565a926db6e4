"""Drive slicer, host side: a numpy restatement of the reference's slicing, clipping and noise
arithmetic (tools/generate_train_data.py:134-182,247-273; tools/augment_train_data.py:18-54) -
plain quaternion algebra, explicit float32 for the radius test - pinned against the g11 fixture the
reference's own functions produced; slice planning, the scene-file writer and the stream's
planning of (item, k) pairs; and the GPU-only functions refusing to run without a GPU.  The GPU
tests (test_drive_gpu.py) hold the HIP kernels to this restatement.

Tolerance: local coordinates, clipped vertices and apply_noise within 1e-9 m absolute.  fp64
rounding of a rotation of a vector of at most 85 m is about 1e-13 (a plain quaternion restatement
against the reference's scipy path: 3.6e-14); 1e-9 leaves four orders of magnitude and is five
below the 1e-4 m the scene files carry.  Membership, order and keep decisions are exact."""
import json
import os

import numpy as np
import pytest
import torch

TOL = 1e-9
HALF = 25.0


def load_g11(golden_dir):
    return np.load(os.path.join(golden_dir, "g11_drive_slices.npz"))


# ------------------------------------------------------------------ the restatement
def inverse_matrix(q):
    """Matrix of the inverse of the normalised quaternion [qx,qy,qz,qw]."""
    x, y, z, w = np.asarray(q, dtype=np.float64) / np.sqrt(np.sum(np.square(np.asarray(q, dtype=np.float64))))
    r = np.array([[x * x - y * y - z * z + w * w, 2 * (x * y - z * w), 2 * (x * z + y * w)],
                  [2 * (x * y + z * w), -x * x + y * y - z * z + w * w, 2 * (y * z - x * w)],
                  [2 * (x * z - y * w), 2 * (y * z + x * w), -x * x - y * y + z * z + w * w]])
    return r.T


def to_local(xyz, pose):
    c = np.asarray(xyz, dtype=np.float64).reshape(-1, 3) - np.asarray(pose[:3], dtype=np.float64)
    m = inverse_matrix(pose[3:7])
    return np.stack([(m[k, 0] * c[:, 0] + m[k, 1] * c[:, 1]) + m[k, 2] * c[:, 2] for k in range(3)], axis=1)


def radius_mask(cloud, pose, radius=60.0):
    """(dx**2 + dy**2) < 3600 as numpy evaluates it on a float32 cloud: float32 throughout."""
    dx = cloud[:, 0].astype(np.float32) - np.float32(pose[0])
    dy = cloud[:, 1].astype(np.float32) - np.float32(pose[1])
    d2 = (dx * dx).astype(np.float32) + (dy * dy).astype(np.float32)
    assert d2.dtype == np.float32
    return d2 < np.float32(radius * radius)


def slice_ref(cloud, poses, half=HALF, radius=60.0, return_margin=False):
    """(points (T,4) fp64, offsets (S+1,), source_index (T,)) [, distance of every emitted-or-not
    disc point to the nearer x-crop plane, as (source rows, margins) per slice]."""
    pts, idx, off, margins = [], [], [0], []
    for pose in np.asarray(poses, dtype=np.float64).reshape(-1, 7):
        rows = np.flatnonzero(radius_mask(cloud, pose, radius))
        local = to_local(cloud[rows, :3], pose)
        keep = (local[:, 0] >= -half) & (local[:, 0] <= half)
        pts.append(np.column_stack([local[keep], cloud[rows[keep], 3].astype(np.float64)]))
        idx.append(rows[keep])
        off.append(off[-1] + int(keep.sum()))
        margins.append((rows, np.abs(np.abs(local[:, 0]) - half)))
    points = np.concatenate(pts) if pts else np.zeros((0, 4))
    index = np.concatenate(idx) if idx else np.zeros(0, dtype=np.int64)
    out = (points, np.array(off, dtype=np.int64), index.astype(np.int64))
    return out + (margins,) if return_margin else out


def clip_ref(points, x_min=-HALF, x_max=HALF):
    """clip_polyline_by_x, generate_train_data.py:145-182."""
    points = np.asarray(points, dtype=np.float64).reshape(-1, 3)
    if len(points) < 2:
        if len(points) == 1 and x_min <= points[0][0] <= x_max:
            return points
        return np.empty((0, 3))
    new = []
    for i in range(len(points) - 1):
        p1, p2 = points[i], points[i + 1]
        t0, t1 = 0.0, 1.0
        dx = p2[0] - p1[0]
        if abs(dx) < 1e-6:
            if p1[0] < x_min or p1[0] > x_max:
                continue
        else:
            t_min, t_max = (x_min - p1[0]) / dx, (x_max - p1[0]) / dx
            if dx > 0:
                t0, t1 = max(t0, t_min), min(t1, t_max)
            else:
                t0, t1 = max(t0, t_max), min(t1, t_min)
        if t0 <= t1:
            pt0, pt1 = p1 + t0 * (p2 - p1), p1 + t1 * (p2 - p1)
            d = new[-1] - pt0 if new else None
            if not new or np.sqrt((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]) > 1e-6:
                new.append(pt0)
            new.append(pt1)
    return np.array(new).reshape(-1, 3)


def clip_lines_ref(lines, poses, half=HALF):
    """counts (S,L) and the clipped polylines [[(k,3)]] of every (pose, line) pair."""
    poses = np.asarray(poses, dtype=np.float64).reshape(-1, 7)
    out = [[clip_ref(to_local(l, p) if len(l) else np.empty((0, 3)), -half, half) for l in lines] for p in poses]
    return np.array([[len(c) for c in row] for row in out], dtype=np.int64).reshape(len(poses), len(lines)), out


def apply_noise_ref(gt, yaw, shift, jitter):
    gt = np.asarray(gt, dtype=np.float64).reshape(-1, 3)
    cen = gt.sum(axis=0) / len(gt)
    c, s = np.cos(yaw), np.sin(yaw)
    p = gt - cen
    rot = np.stack([p[:, 0] * c + p[:, 1] * (-s), p[:, 0] * s + p[:, 1] * c, p[:, 2]], axis=1)
    return rot + cen + np.asarray(shift, dtype=np.float64) + np.asarray(jitter, dtype=np.float64)


def split(verts, lens):
    o = np.concatenate(([0], np.cumsum(lens)))
    return [verts[o[i]:o[i + 1]] for i in range(len(lens))]


# ------------------------------------------------------------------ the fixture
def test_g11_covers_the_cases(golden_dir):
    z = load_g11(golden_dir)
    assert int(z["n_drives"]) == 2
    assert np.abs(z["d1_cloud"][:, :2]).min() > 1e6 and np.abs(z["d1_poses"][:, 0]).min() > 1e6     # UTM-sized
    for d in range(2):
        poses, chosen = z[f"d{d}_poses"], z[f"d{d}_chosen"]
        assert 12 <= len(poses) <= 20 and len(chosen) >= 4
        assert (np.diff(z[f"d{d}_offsets"]) > 0).all()
        x = poses[:, 0]
        steps = np.arange(x.min() + 25.0, x.max(), 25.0)
        gaps = np.abs(x[None, :] - steps[:, None])
        assert (gaps.min(axis=1) > 10.0).any()                                   # a skipped step
        assert ((gaps == gaps.min(axis=1, keepdims=True)).sum(axis=1) > 1).any()   # a tie
        mats = [inverse_matrix(p[3:]).T for p in poses]
        yaw = np.degrees([np.arctan2(m[1, 0], m[0, 0]) for m in mats])
        assert yaw.min() < -120 and yaw.max() > 120 and ((yaw > -60) & (yaw < 60)).any()
        assert (np.abs(np.linalg.norm(poses[:, 3:], axis=1) - 1) > 0.1).any()      # a quaternion to normalise
    d2 = z["d0_boundary_d2"]
    lo, hi = np.nextafter(np.float32(3600), np.float32(0)), np.nextafter(np.float32(3600), np.float32(1e9))
    assert (d2 == lo).any() and (d2 == np.float32(3600)).any() and (d2 == hi).any()
    assert z["d0_boundary_in_radius"].any() and (~z["d0_boundary_in_radius"]).any()
    cnt = z["clip_counts"]
    assert (cnt == 0).any() and (cnt == 1).any() and (cnt == 2).any() and (cnt > 4).any()
    assert set(z["clip_line_len"][:int(z["n_special_lines"])]) >= {0, 1, 2}
    assert z["clip_kept"].any() and (~z["clip_kept"]).any()
    assert len(z["noise_line_len"]) >= 3 and len(z["noise_scales"]) == 3
    assert z["file_pcd_bytes"].size > 100 and z["file_json_bytes"].size > 100
    assert os.path.getsize(os.path.join(golden_dir, "g11_drive_slices.npz")) <= 512 * 1024


def test_restatement_matches_reference_slices(golden_dir):
    z = load_g11(golden_dir)
    for d in range(2):
        cloud, poses = z[f"d{d}_cloud"], z[f"d{d}_poses"][z[f"d{d}_chosen"]]
        pts, off, idx, margins = slice_ref(cloud, poses, return_margin=True)
        assert np.array_equal(off, z[f"d{d}_offsets"])
        assert np.array_equal(idx, z[f"d{d}_source_index"])
        err = np.abs(pts[:, :3] - z[f"d{d}_points"]).max()
        print(f"drive {d}: {len(idx)} points, local xyz max abs err {err:.3e}")
        assert err < TOL
        assert np.array_equal(pts[:, 3].astype(np.float32), cloud[idx, 3])
        assert min(m.min() for _, m in margins) > 1e-6           # what makes exact membership a fair demand


def test_restatement_decides_radius_boundary_as_reference(golden_dir):
    z = load_g11(golden_dir)
    cloud, poses = z["d0_cloud"], z["d0_poses"][z["d0_chosen"]]
    for r, s, want in zip(z["d0_boundary_rows"], z["d0_boundary_slice"], z["d0_boundary_in_radius"]):
        assert bool(radius_mask(cloud[r:r + 1], poses[s])[0]) == bool(want)


def test_restatement_matches_reference_clip(golden_dir):
    z = load_g11(golden_dir)
    lines = split(z["clip_line_verts"], z["clip_line_len"])
    cnt, out = clip_lines_ref(lines, z["clip_poses"])
    assert np.array_equal(cnt, z["clip_counts"])
    assert np.array_equal(cnt > 1, z["clip_kept"])
    got = np.concatenate([c for row in out for c in row])
    err = np.abs(got - z["clip_out_verts"]).max()
    print(f"clip: {cnt.size} pairs, {len(got)} vertices, max abs err {err:.3e}")
    assert err < TOL


def test_restatement_matches_reference_noise(golden_dir):
    z = load_g11(golden_dir)
    lines = split(z["noise_line_verts"], z["noise_line_len"])
    a = 0
    for l, line in enumerate(lines):
        for k in range(len(z["noise_scales"])):
            n = len(line)
            got = apply_noise_ref(line, z["noise_yaw"][l, k], z["noise_shift"][l, k], z["noise_jitter"][a:a + n])
            assert np.abs(got - z["noise_out"][a:a + n]).max() < TOL
            a += n


# ------------------------------------------------------------------ host functions of the package
def test_plan_slices_matches_reference(golden_dir):
    from pointnet_refine_amd import drive
    z = load_g11(golden_dir)
    for d in range(2):
        poses = z[f"d{d}_poses"]
        assert drive.plan_slices(poses) == z[f"d{d}_chosen"].tolist()
        dicts = [{"x": float(p[0]), "y": float(p[1]), "z": float(p[2]), "q": list(p[3:])} for p in poses]
        assert drive.plan_slices(dicts) == z[f"d{d}_chosen"].tolist()
    assert drive.plan_slices([]) == []
    assert drive.plan_slices(np.array([[0.0], [40.0], [80.0]]), max_pose_gap=1.0) == []


def test_load_poses_sorts_and_skips(tmp_path, capsys):
    from pointnet_refine_amd import drive
    for name, x in (("000020", 2.0), ("000003", 1.0)):
        (tmp_path / f"{name}.json").write_text(json.dumps(
            {"x": x, "y": 0.5, "z": 0.1, "qx": 0, "qy": 0, "qz": 0, "qw": 1, **({"ts": 77} if x == 1.0 else {})}))
    (tmp_path / "000010.json").write_text("{not json")
    poses = drive.load_poses(str(tmp_path))
    assert [p["filename_ts"] for p in poses] == ["000003", "000020"]
    assert poses[0]["ts"] == "77" and poses[1]["ts"] == "000020" and poses[0]["q"] == [0, 0, 0, 1]
    assert "000010" in capsys.readouterr().out
    assert drive.poses_xyzq(poses, [1]).tolist() == [[2.0, 0.5, 0.1, 0, 0, 0, 1]]


def test_write_scene_reproduces_reference_bytes(golden_dir, tmp_path):
    from pointnet_refine_amd import drive, io
    z = load_g11(golden_dir)
    meta = json.loads(z["file_item_meta"].tobytes().decode())
    items = [{"category": m["category"], "attributes": m["attributes"], "points": v}
             for m, v in zip(meta, split(z["file_item_verts"], z["file_item_len"]))]
    pcd, js = str(tmp_path / "s.pcd"), str(tmp_path / "s.json")
    drive.write_scene(pcd, js, z["file_points"], items, z["file_ref_ts"].tobytes().decode())
    assert open(pcd, "rb").read() == z["file_pcd_bytes"].tobytes()
    assert open(js, "rb").read() == z["file_json_bytes"].tobytes()
    back = io.load_pcd_data(pcd)
    assert back.shape == (len(z["file_points"]), 4)
    assert np.abs(back[:, :3] - z["file_points"][:, :3]).max() < 1e-4
    assert np.array_equal(back[:, 3], np.trunc(z["file_points"][:, 3]).astype(np.float32))
    read = io.load_scene_items(js)
    assert len(read) == len(items)
    for r, it in zip(read, items):
        assert np.array_equal(r["position"], it["points"]) and r["noisy_candidates"] == []


def _gt_only_scene(root, name, n_items=3):
    from pointnet_refine_amd import drive
    rng = np.random.default_rng(5)
    pts = np.column_stack([rng.uniform(-25, 25, 300), rng.uniform(-8, 8, 300), rng.uniform(-1, 1, 300),
                           rng.uniform(0, 255, 300)])
    items = [{"category": "lane", "attributes": {}, "points": np.column_stack(
        [np.linspace(-20, 20, 9), np.full(9, 3.0 * i), np.zeros(9)])} for i in range(n_items)]
    items.append({"category": "lane", "attributes": {}, "points": np.array([[0.0, 0.0, 0.0]])})   # 1 vertex: never drawn
    drive.write_scene(os.path.join(root, name + ".pcd"), os.path.join(root, name + ".json"), pts, items, name)


def test_stream_plans_augmented_pairs_for_gt_only_scenes(tmp_path):
    from pointnet_refine_amd.io import SceneSampleStream
    _gt_only_scene(str(tmp_path), "000001")
    _gt_only_scene(str(tmp_path), "000002", n_items=2)
    plain = SceneSampleStream(str(tmp_path), device="cpu", batch_size=4)
    assert len(plain) == 0 and plain._plan() == []               # GT only: nothing to train on without augment
    st = SceneSampleStream(str(tmp_path), device="cpu", batch_size=4, augment=(0.1, 0.25, 0.4), shuffle=False)
    assert len(st) == (3 + 2) * 3
    assert [s[2] for s in st.scenes] == [[(i, k) for i in range(3) for k in range(3)],
                                         [(i, k) for i in range(2) for k in range(3)]]
    plan = st._plan()
    assert sorted(p for _, prs in plan for p in prs) == sorted(p for s in st.scenes for p in s[2])
    halves = [SceneSampleStream(str(tmp_path), device="cpu", augment=(0.2, 0.3), rank=r, world_size=2) for r in (0, 1)]
    assert len(halves[0]) == len(halves[1]) == 5
    with pytest.raises(ValueError):
        SceneSampleStream(str(tmp_path), device="cpu", augment=())


def test_drive_refuses_to_run_without_gpu(monkeypatch):
    from pointnet_refine_amd import drive
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    pose = np.array([[0, 0, 0, 0, 0, 0, 1.0]])
    line = np.array([[-1.0, 0, 0], [1.0, 0, 0]])
    with pytest.raises(RuntimeError, match="GPU"):
        drive.slice_cloud(np.zeros((4, 4), np.float32), pose)
    with pytest.raises(RuntimeError, match="GPU"):
        drive.clip_lines([line], pose)
    with pytest.raises(RuntimeError, match="GPU"):
        drive.apply_noise(line, 0.01, np.zeros(3), np.zeros((2, 3)))
    with pytest.raises(RuntimeError, match="GPU"):
        drive.noisy_candidates([line])
