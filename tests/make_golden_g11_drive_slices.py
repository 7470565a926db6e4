"""Writes tests/golden/g11_drive_slices.npz from the reference's own data-preparation tools
(tools/generate_train_data.py: process_dataset, transform_to_local, clip_polyline_by_x, save_pcd,
save_json; tools/augment_train_data.py: generate_noisy_line).  Not collected by pytest; needs the
reference tree, scipy and tqdm.  The fixture holds inputs and the reference's outputs only.

    python tests/make_golden_g11_drive_slices.py --reference REFERENCE_CHECKOUT

Both tools are loaded by file path; their main() is never called.  Each synthetic drive is written
to a temporary directory (pose/*.json, a binary merged.pcd, a GT JSON) and cut by the reference's
process_dataset with save_pcd / save_json replaced by recorders, so the fixture keeps the fp64
final_points of every slice and the pose process_dataset chose for it.  The cloud's fourth column
carries the row number through the reference's masks (exact in float32 below 2^24): that is the
source index; the intensities the tests use are stored beside it.  The maker asserts that no
point of a 60 m disc lies within 1e-6 m of an x-crop plane, which lets the tests demand exact
membership."""
import argparse
import importlib.util
import io
import json
import os
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "tests", "golden", "g11_drive_slices.npz")
SCALES = (0.1, 0.25, 0.4)
POSE_X = [0, 12, 22, 28, 40, 52, 63, 77, 88, 113, 124, 137, 150, 161, 175, 190]
# steps at 25, 50, ...: 25 ties between the poses at 22 and 28 (the first wins); 100 is 12 m from
# the nearest pose (88) and is skipped


def load_tool(ref_dir, name):
    spec = importlib.util.spec_from_file_location("ref_" + name, os.path.join(ref_dir, "tools", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def make_drive(seed, origin, n_points):
    from scipy.spatial.transform import Rotation as R
    rng = np.random.default_rng(seed)
    ox, oy, oz = origin
    n = len(POSE_X)
    px = np.array(POSE_X, dtype=np.float64) + ox
    py = oy + 6.0 * np.sin(np.array(POSE_X) / 40.0) + rng.uniform(-0.3, 0.3, n)
    pz = oz + 0.02 * np.array(POSE_X) + rng.uniform(-0.1, 0.1, n)
    yaw = (np.arange(n) * (360.0 / n) + rng.uniform(-8, 8, n)) % 360.0 - 180.0       # the full circle
    pitch, roll = rng.uniform(-3, 3, n), rng.uniform(-3, 3, n)
    q = R.from_euler("zyx", np.stack([yaw, pitch, roll], 1), degrees=True).as_quat()
    q[3] *= 1.7                                                                     # not normalised
    q[9] *= -0.6
    poses = np.column_stack([px, py, pz, q])
    x = rng.uniform(-70, 260, n_points) + ox
    y = oy + 6.0 * np.sin((x - ox) / 40.0) + rng.uniform(-75, 75, n_points)
    z = oz + rng.uniform(-2, 6, n_points)
    inten = np.round(rng.uniform(-3, 255, n_points), 2)
    cloud = np.column_stack([x, y, z, inten]).astype(np.float32)
    return poses, cloud


def boundary_points(rng, G, pose, want=4):
    """float32 points whose float32 dx*dx + dy*dy is the float32 just below, equal to and just above
    3600, inside the pose's x-crop.  Returns (points (m,3) float32, d2 (m,) float32)."""
    lo, hi = np.nextafter(np.float32(3600), np.float32(0)), np.nextafter(np.float32(3600), np.float32(1e9))
    pd = {"x": float(pose[0]), "y": float(pose[1]), "z": float(pose[2]), "q": list(pose[3:])}
    th = rng.uniform(0, 2 * np.pi, 400000)
    x = (pose[0] + 60.0 * np.cos(th)).astype(np.float32)
    y = (pose[1] + 60.0 * np.sin(th)).astype(np.float32)
    for _ in range(3):                                       # walk a few float32 steps around the circle
        x = np.concatenate([x, np.nextafter(x, np.float32(1e9)), np.nextafter(x, np.float32(-1e9))])
        y = np.concatenate([y, y, y])
    z = np.full(len(x), pose[2], dtype=np.float32)
    dx = x - pd["x"]
    dy = y - pd["y"]
    d2 = dx ** 2 + dy ** 2
    assert d2.dtype == np.float32
    local = G.transform_to_local(np.column_stack([x, y, z]), pd)
    inside = np.abs(local[:, 0]) < 24.0
    pts, vals = [], []
    for target in (lo, np.float32(3600), hi):
        idx = np.flatnonzero((d2 == target) & inside)
        assert len(idx) >= 1, f"no boundary point with d2 == {target!r}"
        idx = idx[:want]
        pts.append(np.column_stack([x[idx], y[idx], z[idx]]))
        vals.append(d2[idx])
    return np.concatenate(pts).astype(np.float32), np.concatenate(vals)


def run_reference_drive(G, poses, cloud_idx, lanes):
    """process_dataset on a temporary drive; returns [(pose file name, final_points fp64)]."""
    got = []
    with tempfile.TemporaryDirectory() as tmp:
        drive = os.path.join(tmp, "d_annotation_raw_data")
        os.makedirs(os.path.join(drive, "pose"))
        for i, p in enumerate(poses):
            with open(os.path.join(drive, "pose", f"{1000 + i:06d}.json"), "w") as f:
                json.dump({"x": float(p[0]), "y": float(p[1]), "z": float(p[2]), "qx": float(p[3]),
                           "qy": float(p[4]), "qz": float(p[5]), "qw": float(p[6])}, f)
        assert (len(cloud_idx) * 16) % 14 != 0          # or load_pcd_fast takes the 14-byte layout
        with open(os.path.join(drive, "merged.pcd"), "wb") as f:
            f.write((f"VERSION 0.7\nFIELDS x y z intensity\nSIZE 4 4 4 4\nTYPE F F F F\nCOUNT 1 1 1 1\n"
                     f"WIDTH {len(cloud_idx)}\nHEIGHT 1\nVIEWPOINT 0 0 0 1 0 0 0\nPOINTS {len(cloud_idx)}\n"
                     "DATA binary\n").encode())
            f.write(np.ascontiguousarray(cloud_idx, dtype="<f4").tobytes())
        gt = os.path.join(tmp, "d.bag.json")
        with open(gt, "w") as f:
            json.dump({"items": [{"category": "lane", "attributes": {"id": i},
                                  "position": [{"x": float(a), "y": float(b), "z": float(c)} for a, b, c in l]}
                                 for i, l in enumerate(lanes)]}, f)
        keep_pcd, keep_json = G.save_pcd, G.save_json
        G.save_pcd = lambda path, points: got.append((os.path.splitext(os.path.basename(path))[0],
                                                      np.array(points, dtype=np.float64)))
        G.save_json = lambda path, items, ref_ts: None
        try:
            G.process_dataset(drive, gt, tmp)
        finally:
            G.save_pcd, G.save_json = keep_pcd, keep_json
    return got


def clip_lines_cases():
    P = lambda *p: np.array(p, dtype=np.float64).reshape(-1, 3)
    return [
        P((-40, 1, 0), (40, 2, 0.5)),                                          # crosses both planes
        P((-40, 3, 0), (-10, 3, 0), (10, 40, 0), (40, 41, 0), (10, 42, 0), (-40, 43, 0)),   # leaves and re-enters
        P((-20, 5, 0), (-5, 5.5, 0), (5, 5, 0), (20, 5.5, 0)),                 # entirely inside
        P((30, 7, 0), (45, 7, 0), (60, 8, 0)),                                 # entirely outside
        P((-30, 9, 0), (-25, 9, 0), (0, 9, 0), (25, 9.5, 0), (30, 9, 0)),      # vertices exactly on the planes
        P((10, 11, 0), (10, 15, 0), (10, 19, 1)),                              # constant x, inside
        P((30, 11, 0), (30, 15, 0), (20, 16, 0)),                              # constant x outside, then in
        P((-5, 13, 0), (0, 13, 0), (0, 13, 0), (5, 13, 0), (5, 13, 0), (5, 13, 0), (12, 13, 0)),   # duplicates
        np.empty((0, 3)),                                                      # 0 vertices
        P((3, 17, 0)),                                                         # 1 vertex inside
        P((33, 17, 0)),                                                        # 1 vertex outside
        P((-3, 19, 0), (4, 19, 0)),                                            # 2 vertices
        P((40, 21, 0), (10, 21.5, 0), (-10, 21, 0), (-40, 21.5, 0)),           # reversed direction
        P((24.9999999, 23, 0), (25.0000004, 23, 0), (26, 24, 0)),              # |dx| < 1e-6 straddling a plane
        P((-60, 25, 0), (60, 25, 0), (60, 26, 0), (-60, 26, 0)),               # out and back across the slice
    ]


def lanes_for(poses, seed):
    rng = np.random.default_rng(seed)
    ox, oy, oz = poses[0, 0], poses[0, 1] - 0.0, poses[0, 2]
    lanes = []
    for k in range(5):
        n = int(rng.integers(20, 70))
        x = np.sort(rng.uniform(-30, 230, n)) + ox
        if k % 2:
            x = x[::-1]
        y = oy + 6.0 * np.sin((x - ox) / 40.0) + 3.5 * (k - 2) + rng.normal(0, 0.05, n)
        z = oz + 0.02 * (x - ox) + rng.normal(0, 0.02, n)
        lanes.append(np.column_stack([x, y, z]))
    return lanes


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True, help="checkout of the reference repository")
    args = ap.parse_args()
    G = load_tool(args.reference, "generate_train_data")
    A = load_tool(args.reference, "augment_train_data")
    out = {}
    rng = np.random.default_rng(11)

    # ---- drives: slices of the cloud
    all_poses, all_lanes = [], []
    for d, (origin, n_points) in enumerate((((0.0, 0.0, 0.0), 2000), ((1.2e6, 5.1e6, 35.0), 2000))):
        poses, cloud = make_drive(100 + d, origin, n_points)
        plan_guess = [2, 5, 7, 10, 12, 14]          # the poses the walk is expected to pick; checked below
        bp, bd2, bslice = [], [], []
        # (float32 steps at UTM-sized coordinates are 0.125 m and more: no d2 next to 3600 exists there)
        for s in ((0, 3) if d == 0 else ()):
            p, v = boundary_points(rng, G, poses[plan_guess[s]])
            bp.append(p); bd2.append(v); bslice.append(np.full(len(p), s))
        bp = np.concatenate(bp) if bp else np.zeros((0, 3), dtype=np.float32)
        bd2.append(np.zeros(0, dtype=np.float32)); bslice.append(np.zeros(0, dtype=np.int64))
        b_int = np.round(rng.uniform(0, 200, len(bp)), 1).astype(np.float32)
        boundary_rows = np.arange(len(cloud), len(cloud) + len(bp))
        cloud = np.concatenate([cloud, np.column_stack([bp, b_int]).astype(np.float32)])
        if len(cloud) % 7 == 0:
            cloud = np.concatenate([cloud, cloud[:1]])
        lanes = lanes_for(poses, 200 + d)
        cloud_idx = cloud.copy()
        cloud_idx[:, 3] = np.arange(len(cloud), dtype=np.float32)
        got = run_reference_drive(G, poses, cloud_idx, lanes)
        names = [f"{1000 + i:06d}" for i in range(len(poses))]
        chosen = [names.index(n) for n, _ in got]
        assert chosen == plan_guess, chosen
        pts, src, off = [], [], [0]
        for (name, fp), j in zip(got, chosen):
            idx = fp[:, 3].astype(np.int64)
            assert np.all(np.diff(idx) > 0)
            pts.append(fp[:, :3]); src.append(idx); off.append(off[-1] + len(fp))
            pd = {"x": float(poses[j, 0]), "y": float(poses[j, 1]), "z": float(poses[j, 2]), "q": list(poses[j, 3:])}
            dx = cloud[:, 0] - pd["x"]
            dy = cloud[:, 1] - pd["y"]
            near = (dx ** 2 + dy ** 2) < 3600
            local = G.transform_to_local(cloud[near], pd)
            assert np.abs(np.abs(local[:, 0]) - 25.0).min() > 1e-6, "a point within 1e-6 m of an x-crop plane"
        # the radius decision of the boundary points, as the reference's expression gives it
        b_in = []
        for r, s in zip(boundary_rows, np.concatenate(bslice)):
            j = chosen[s]
            dx = cloud[r:r + 1, 0] - float(poses[j, 0])
            dy = cloud[r:r + 1, 1] - float(poses[j, 1])
            b_in.append(bool(((dx ** 2 + dy ** 2) < 3600)[0]))
        pre = f"d{d}_"
        out[pre + "poses"] = poses
        out[pre + "cloud"] = cloud
        out[pre + "chosen"] = np.array(chosen, dtype=np.int64)
        out[pre + "points"] = np.concatenate(pts)
        out[pre + "source_index"] = np.concatenate(src)
        out[pre + "offsets"] = np.array(off, dtype=np.int64)
        out[pre + "boundary_rows"] = boundary_rows
        out[pre + "boundary_slice"] = np.concatenate(bslice)
        out[pre + "boundary_d2"] = np.concatenate(bd2)
        out[pre + "boundary_in_radius"] = np.array(b_in)
        all_poses.append(poses[chosen]); all_lanes.append(lanes)
        print(f"drive {d}: {len(cloud)} points, poses {chosen}, slice sizes {np.diff(off).tolist()}, "
              f"boundary in-radius {np.array(b_in).astype(int).tolist()}")
    out["n_drives"] = np.int64(2)

    # ---- polylines: clip_polyline_by_x in every frame
    clip_poses = np.concatenate([np.array([[0, 0, 0, 0, 0, 0, 1.0]]), all_poses[0], all_poses[1]])
    lines = clip_lines_cases() + all_lanes[0] + all_lanes[1]
    counts = np.zeros((len(clip_poses), len(lines)), dtype=np.int64)
    verts = []
    for s, p in enumerate(clip_poses):
        pd = {"x": float(p[0]), "y": float(p[1]), "z": float(p[2]), "q": list(p[3:])}
        for l, line in enumerate(lines):
            clipped = G.clip_polyline_by_x(G.transform_to_local(line, pd), -G.SEGMENT_LEN / 2, G.SEGMENT_LEN / 2)
            clipped = np.asarray(clipped, dtype=np.float64).reshape(-1, 3)
            counts[s, l] = len(clipped)
            verts.append(clipped)
    out["clip_poses"] = clip_poses
    out["clip_line_verts"] = np.concatenate(lines)
    out["clip_line_len"] = np.array([len(l) for l in lines], dtype=np.int64)
    out["clip_counts"] = counts
    out["clip_kept"] = counts > 1                         # process_dataset's len(clipped) > 1
    out["clip_out_verts"] = np.concatenate(verts)
    out["n_special_lines"] = np.int64(len(clip_lines_cases()))
    print(f"clip: {counts.size} (pose, line) pairs, {int((counts > 1).sum())} kept, "
          f"{int((counts == 1).sum())} single-vertex, {int((counts == 0).sum())} empty")

    # ---- generate_noisy_line with replayed draws
    noise_lines = [all_lanes[0][0][:2], all_lanes[0][1][:10], all_lanes[1][2][:40]]
    n_yaw, n_shift, n_jit, n_out = [], [], [], []
    for l, line in enumerate(noise_lines):
        dicts = [{"x": float(a), "y": float(b), "z": float(c)} for a, b, c in line]
        for k, s in enumerate(SCALES):
            seed = 10 * l + k
            np.random.seed(seed)
            ref = A.generate_noisy_line(dicts, noise_scale=s)
            ref = np.array([[p["x"], p["y"], p["z"]] for p in ref])
            np.random.seed(seed)                        # replay: uniform x4, then normal x3 per vertex
            yaw = np.random.uniform(-5.0 * s, 5.0 * s) * (np.pi / 180.0)
            shift = np.array([np.random.uniform(-s, s), np.random.uniform(-s, s), np.random.uniform(-0.1, 0.1)])
            jit = np.array([[np.random.normal(0, 0.05), np.random.normal(0, 0.05), np.random.normal(0, 0.025)]
                            for _ in line])
            c, sn = np.cos(yaw), np.sin(yaw)
            rot = np.array([[c, -sn, 0], [sn, c, 0], [0, 0, 1]])
            cen = np.mean(line, axis=0)
            again = (line - cen) @ rot.T + cen + shift + jit
            assert np.abs(again - ref).max() < 1e-9, "replayed draws do not reproduce generate_noisy_line"
            n_yaw.append(yaw); n_shift.append(shift); n_jit.append(jit); n_out.append(ref)
    out["noise_line_verts"] = np.concatenate(noise_lines)
    out["noise_line_len"] = np.array([len(l) for l in noise_lines], dtype=np.int64)
    out["noise_scales"] = np.array(SCALES)
    out["noise_yaw"] = np.array(n_yaw).reshape(len(noise_lines), len(SCALES))
    out["noise_shift"] = np.array(n_shift).reshape(len(noise_lines), len(SCALES), 3)
    out["noise_jitter"] = np.concatenate(n_jit)           # (line, scale) blocks in order
    out["noise_out"] = np.concatenate(n_out)

    # ---- the bytes save_pcd / save_json write for one small slice
    o = out["d0_offsets"]
    sl = out["d0_points"][o[0]:o[0] + 40]
    pts4 = np.column_stack([sl, out["d0_cloud"][out["d0_source_index"][o[0]:o[0] + 40], 3].astype(np.float64)])
    items = []
    for l in range(len(lines)):
        if counts[1, l] > 1 and len(items) < 3:           # clip pose 1 = drive 0, slice 0
            a = int(counts[:1].sum() + counts[1, :l].sum())
            items.append({"category": ["lane", "curb", "stop_line"][len(items)],
                          "attributes": {"id": l, "color": "white"} if len(items) != 1 else {},
                          "points": out["clip_out_verts"][a:a + counts[1, l]]})
    with tempfile.TemporaryDirectory() as tmp:
        G.save_pcd(os.path.join(tmp, "s.pcd"), pts4)
        G.save_json(os.path.join(tmp, "s.json"), items, "001002")
        out["file_pcd_bytes"] = np.frombuffer(open(os.path.join(tmp, "s.pcd"), "rb").read(), dtype=np.uint8)
        out["file_json_bytes"] = np.frombuffer(open(os.path.join(tmp, "s.json"), "rb").read(), dtype=np.uint8)
    out["file_points"] = pts4
    out["file_item_verts"] = np.concatenate([it["points"] for it in items])
    out["file_item_len"] = np.array([len(it["points"]) for it in items], dtype=np.int64)
    out["file_item_meta"] = np.frombuffer(json.dumps([{"category": it["category"], "attributes": it["attributes"]}
                                                      for it in items]).encode(), dtype=np.uint8)
    out["file_ref_ts"] = np.frombuffer(b"001002", dtype=np.uint8)

    buf = io.BytesIO()
    np.savez_compressed(buf, **out)
    assert buf.tell() <= 512 * 1024, buf.tell()
    with open(OUT, "wb") as f:
        f.write(buf.getvalue())
    print(f"wrote {OUT} ({buf.tell()} bytes)")


if __name__ == "__main__":
    main()
