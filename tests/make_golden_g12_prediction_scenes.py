"""Writes tests/golden/g12_prediction_scenes.npz from the reference's own prediction-scene tool
(tools/generate_inference_data_vma.py).  Not collected by pytest; needs the reference tree and
scipy.  The fixture holds inputs and the reference's outputs only.

    python tests/make_golden_g12_prediction_scenes.py --reference REFERENCE_CHECKOUT

The tool's matching is inline in main(), so the maker loads the tool by file path, points its
module constants at a temporary synthetic drive (pose/*.json, a merged.pcd in the 14-byte
f4 f4 f4 u2 layout the tool reads, a GT JSON, a detector-results JSON), calls main() and reads back
the files it wrote.  The cloud's intensity carries the row number (< 65536), which is the source
index of every written point; the PCD carries 1e-4 m, so the fp64 points stored are
transform_to_local's, checked against the file.  JSON floats round-trip exactly: context_lines and
position are the reference's fp64.  The matched GT of an item is recovered by comparing position
with context_lines; the cost matrices are recomputed with the tool's expression and asserted to
reproduce, through scipy, every match the tool wrote.

Conditions asserted so the tests may demand exact decisions: in every stored frame but the tie
frame the optimal assignment is unique by a margin (forbidding any matched pair raises the optimum
by >= 1e-6); no matched cost within 1e-6 of 15.0; no cloud point of a disc within 1e-6 m of a crop
plane; no GT vertex within 1e-6 m of |x| = 25 - except the two ends of the one designed segment
with |dx| < 1e-6 across a plane, which cannot satisfy that and lie >= 2e-7 m from it instead (five
orders above the 1e-12 m rounding of the transform)."""
import argparse
import importlib.util
import io
import json
import os
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "tests", "golden", "g12_prediction_scenes.npz")
ORIGIN = np.array([4.0e5, 5.0e6, 30.0])
T0 = 1_755_661_956_000_000_000          # ns; above 2^53
STEP = 100_000_000                      # a pose every 100 ms
N_ROAD = 12                             # poses along the road; 12.. are the islands
ISLANDS = {"one": 12, "none": 13, "crop": 14, "tie": 15, "disc": 16}


def load_tool(ref_dir):
    spec = importlib.util.spec_from_file_location(
        "ref_vma", os.path.join(ref_dir, "tools", "generate_inference_data_vma.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def pose_dict(p):
    return {"x": float(p[0]), "y": float(p[1]), "z": float(p[2]), "q": [float(v) for v in p[3:]]}


def to_global(local, pose):
    """Inverse of the tool's transform_to_local, for placing designed vertices in a frame."""
    from scipy.spatial.transform import Rotation as R
    return R.from_quat(pose[3:]).apply(np.asarray(local, dtype=np.float64)) + pose[:3]


def make_world(G, rng):
    from scipy.spatial.transform import Rotation as R
    n = N_ROAD + len(ISLANDS)
    xs = np.concatenate([12.0 * np.arange(N_ROAD), 1000.0 + 400.0 * np.arange(len(ISLANDS))])
    pos = np.column_stack([ORIGIN[0] + xs, ORIGIN[1] + 5.0 * np.sin(xs / 40.0) + rng.uniform(-0.3, 0.3, n),
                           ORIGIN[2] + 0.01 * xs])
    yaw = (np.arange(n) * (360.0 / N_ROAD) + rng.uniform(-8, 8, n)) % 360.0 - 180.0      # the full circle
    q = R.from_euler("zyx", np.stack([yaw, rng.uniform(-3, 3, n), rng.uniform(-3, 3, n)], 1), degrees=True).as_quat()
    poses = np.column_stack([pos, q])
    assert np.abs(np.sqrt((q ** 2).sum(1)) - 1).max() < 1e-15
    lanes = []
    for k in range(5):                                          # the road: five lanes 3.5 m apart
        m = int(rng.integers(30, 60))
        x = np.sort(rng.uniform(-40, 12.0 * N_ROAD + 40, m))
        if k % 2:
            x = x[::-1]
        lanes.append(np.column_stack([ORIGIN[0] + x, ORIGIN[1] + 5.0 * np.sin(x / 40.0) + 3.5 * (k - 2) +
                                      rng.normal(0, 0.05, m), ORIGIN[2] + 0.01 * x + rng.normal(0, 0.02, m)]))
    # crosses the slab of pose 3 without a vertex strictly inside: dropped by this tool
    lanes.append(to_global([(-40.0, 12.0, 0.0), (40.0, 13.0, 0.1)], poses[3]))
    # |dx| < 1e-6 across the +25 plane of pose 9
    lanes.append(to_global([(8.0, -13.5, 0.0), (24.9999997, -14.0, 0.0), (25.0000004, -14.5, 0.1), (27.0, -15.0, 0.0)],
                           poses[9]))
    special_dx = len(lanes) - 1
    p = poses[ISLANDS["one"]]
    lanes.append(to_global(np.column_stack([np.linspace(-35, 33, 24), 2.0 + rng.normal(0, 0.1, 24), np.zeros(24)]), p))
    p = poses[ISLANDS["tie"]]
    twin = to_global(np.column_stack([np.linspace(-30, 31, 20), -1.5 + rng.normal(0, 0.1, 20), np.zeros(20)]), p)
    lanes += [twin, twin.copy(),
              to_global(np.column_stack([np.linspace(-28, 29, 18), 2.5 + rng.normal(0, 0.1, 18), np.zeros(18)]), p)]
    # cloud: the road corridor, and a cluster per island (crop: outside |x| <= 25; disc: none at all)
    m = 2600
    x = rng.uniform(-60, 12.0 * N_ROAD + 60, m)
    parts = [np.column_stack([ORIGIN[0] + x, ORIGIN[1] + 5.0 * np.sin(x / 40.0) + rng.uniform(-45, 45, m),
                              ORIGIN[2] + rng.uniform(-2, 5, m)])]
    for name, lo, hi in (("one", -30, 30), ("none", -30, 30), ("crop", 32, 50), ("tie", -30, 30)):
        loc = np.column_stack([rng.uniform(lo, hi, 120), rng.uniform(-20, 20, 120), rng.uniform(-1, 3, 120)])
        parts.append(to_global(loc, poses[ISLANDS[name]]))
    xyz = np.concatenate(parts).astype(np.float32)
    assert len(xyz) < 65536
    cloud = np.column_stack([xyz, np.arange(len(xyz), dtype=np.float32)]).astype(np.float32)
    return poses, lanes, cloud, special_dx


def clip_frame(G, lanes, pose):
    """The tool's gate + clip + keep rule for one pose: [(lane index, (k,3))]."""
    half = G.SEGMENT_LEN / 2
    pd, out = pose_dict(pose), []
    for l, lane in enumerate(lanes):
        loc = G.transform_to_local(lane, pd)
        if np.any((loc[:, 0] > -half) & (loc[:, 0] < half)):
            c = G.clip_polyline_by_x(loc, -half, half)
            if len(c) > 1:
                out.append((l, np.asarray(c, dtype=np.float64).reshape(-1, 3)))
    return out


def to_pixels(xy):
    return np.column_stack([(25.0 - xy[:, 1]) / 0.05, (25.0 - xy[:, 0]) / 0.05])


def from_gt(rng, line, shift=0.4):
    """A detector-like polyline: a resampled stretch of a clipped GT line, shifted and jittered."""
    m = int(rng.integers(8, 30))
    t = np.sort(rng.uniform(0, len(line) - 1, m))
    i = np.minimum(t.astype(int), len(line) - 2)
    xy = line[i, :2] + (t - i)[:, None] * (line[i + 1, :2] - line[i, :2])
    return to_pixels(xy + rng.uniform(-shift, shift, 2) + rng.normal(0, 0.05, (m, 2)))


def clutter(rng):
    m = int(rng.integers(2, 12))
    a, b = rng.uniform(-24, 24, 2), rng.uniform(-24, 24, 2)
    return to_pixels(a + np.linspace(0, 1, m)[:, None] * (b - a) + rng.normal(0, 0.1, (m, 2)))


def tool_cost(pred_lines, gt_lines):
    """:432-448 verbatim on arrays."""
    cost = np.full((len(pred_lines), len(gt_lines)), 1000.0)
    for i, p in enumerate(pred_lines):
        for j, g in enumerate(gt_lines):
            diff = p[:, None, :2] - g[None, :, :2]
            cost[i, j] = np.mean(np.min(np.linalg.norm(diff, axis=2), axis=1))
    return cost


def main():
    from scipy.optimize import linear_sum_assignment
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True, help="checkout of the reference repository")
    args = ap.parse_args()
    G = load_tool(args.reference)
    rng = np.random.default_rng(12)
    poses, lanes, cloud, special_dx = make_world(G, rng)
    n_pose = len(poses)
    pose_ts = [T0 + STEP * i for i in range(n_pose)]
    # islands get timestamps of their own, 1 s apart, so no road frame can reach them
    for k, j in enumerate(ISLANDS.values()):
        pose_ts[j] = T0 + STEP * N_ROAD + 1_000_000_000 * (k + 1)
    pose_names = [str(t) for t in pose_ts]
    pose_names[1] = "pose_b"                       # not an integer: the tool falls back to the file's 'ts'
    clipped = [clip_frame(G, lanes, p) for p in poses]

    # ---- the frames: (result ts, pose it should find or -1, what it holds)
    frames = []

    def add(ts, pose, pixels, scores=None):
        frames.append({"ts": int(ts), "pose": pose, "pixels": pixels,
                       "scores": scores if scores is not None else [round(float(rng.uniform(0.3, 1)), 4) for _ in pixels]})

    gt_of = lambda j: [v for _, v in clipped[j]]
    g = gt_of(0)                                                              # P > G
    add(pose_ts[0] + 3_000_000, 0, [from_gt(rng, l) for l in g] + [clutter(rng) for _ in range(3)])
    g = gt_of(2)                                                              # P < G
    add(pose_ts[2] - 7_000_000, 2, [from_gt(rng, g[k]) for k in (3, 0, 2)])
    g = gt_of(4)                                                              # P = G, shuffled
    add(pose_ts[4] + 1, 4, [from_gt(rng, g[k]) for k in rng.permutation(len(g))])
    g = gt_of(5)                                                              # exactly between poses 5 and 6
    add((pose_ts[5] + pose_ts[6]) // 2, 5, [from_gt(rng, g[1]), from_gt(rng, g[4]), clutter(rng)], [0.9, None, 0.5])
    add(pose_ts[ISLANDS["one"]] + 5, ISLANDS["one"], [from_gt(rng, gt_of(ISLANDS["one"])[0])])      # 1 x 1
    add(pose_ts[ISLANDS["none"]] - 5, ISLANDS["none"], [clutter(rng), clutter(rng)])                # G = 0
    g = gt_of(7)                                                              # one prediction > 15 m from every GT
    far = to_pixels(np.column_stack([np.linspace(-20, 20, 9), np.full(9, 60.0)]))
    add(pose_ts[7] + 11, 7, [from_gt(rng, g[0]), far, from_gt(rng, g[3])])
    g = gt_of(8)                                                              # a one-vertex instance: dropped
    add(pose_ts[8] + 2, 8, [from_gt(rng, g[2]), np.array([[500.0, 500.0]]), from_gt(rng, g[1])])
    add(pose_ts[0] - 250_000_001, -1, [clutter(rng)])                         # no pose within 250 ms
    add(pose_ts[N_ROAD - 1] + 250_000_000, N_ROAD - 1, [from_gt(rng, gt_of(N_ROAD - 1)[2]), clutter(rng)])   # exactly 250 ms
    add(pose_ts[ISLANDS["crop"]], ISLANDS["crop"], [clutter(rng)])            # disc not empty, crop empty
    add(pose_ts[ISLANDS["disc"]], ISLANDS["disc"], [clutter(rng)])            # disc empty
    g = gt_of(3)                                                              # the slab-crossing line is dropped here
    add(pose_ts[3] + 9, 3, [from_gt(rng, l) for l in g[:4]] + [clutter(rng)])
    g = gt_of(9)                                                              # the |dx| < 1e-6 segment
    add(pose_ts[9] - 9, 9, [from_gt(rng, l) for l in g])
    add(pose_ts[10], 10, [])                                                  # no predictions: nothing written
    g = gt_of(ISLANDS["tie"])                                                 # two identical GT lines
    tie_ts = pose_ts[ISLANDS["tie"]] + 77
    add(tie_ts, ISLANDS["tie"], [from_gt(rng, g[0]), from_gt(rng, g[2]), from_gt(rng, g[1])])
    assert special_dx in [l for l, _ in clipped[9]] and 5 not in [l for l, _ in clipped[3]]
    results = {"misc/not_a_frame.jpg": {"pred_instances": []}}
    for fr in frames:
        inst = []
        for px, sc in zip(fr["pixels"], fr["scores"]):
            d = {"data": [[float(u), float(v)] for u, v in px]}
            if sc is not None:
                d["score"] = sc
            inst.append(d)
        results[f"cam/front/{fr['ts']}.jpg"] = {"pred_instances": inst}

    # ---- run the tool
    written = {}
    with tempfile.TemporaryDirectory() as tmp:
        os.makedirs(os.path.join(tmp, "pose"))
        for p, ts, name in zip(poses, pose_ts, pose_names):
            with open(os.path.join(tmp, "pose", name + ".json"), "w") as f:
                json.dump({"ts": str(ts), "x": float(p[0]), "y": float(p[1]), "z": float(p[2]), "qx": float(p[3]),
                           "qy": float(p[4]), "qz": float(p[5]), "qw": float(p[6])}, f)
        rec = np.zeros(len(cloud), dtype=np.dtype([("x", "<f4"), ("y", "<f4"), ("z", "<f4"), ("i", "<u2")]))
        rec["x"], rec["y"], rec["z"], rec["i"] = cloud[:, 0], cloud[:, 1], cloud[:, 2], cloud[:, 3].astype(np.uint16)
        with open(os.path.join(tmp, "merged.pcd"), "wb") as f:
            f.write((f"VERSION 0.7\nFIELDS x y z intensity\nSIZE 4 4 4 2\nTYPE F F F U\nCOUNT 1 1 1 1\n"
                     f"WIDTH {len(cloud)}\nHEIGHT 1\nVIEWPOINT 0 0 0 1 0 0 0\nPOINTS {len(cloud)}\n"
                     "DATA binary\n").encode())
            f.write(rec.tobytes())
        gt_doc = {"items": []}
        for i, l in enumerate(lanes):
            pos = [{"x": float(a), "y": float(b), "z": float(c)} for a, b, c in l]
            gt_doc["items"].append({"category": "lane", "attributes": {"id": i}, "position": pos} if i % 3 else
                                   {"category": "curb", "semantic_line": {"position": pos}})
        with open(os.path.join(tmp, "gt.json"), "w") as f:
            json.dump(gt_doc, f)
        results_bytes = json.dumps(results).encode()
        with open(os.path.join(tmp, "results.json"), "wb") as f:
            f.write(results_bytes)
        G.POSE_DIR, G.PCD_PATH = os.path.join(tmp, "pose"), os.path.join(tmp, "merged.pcd")
        G.GT_JSON_PATH, G.RESULTS_JSON_PATH = os.path.join(tmp, "gt.json"), os.path.join(tmp, "results.json")
        G.OUTPUT_DIR = os.path.join(tmp, "out")
        G.main()
        tool_poses = G.load_poses(G.POSE_DIR)
        for name in sorted(os.listdir(G.OUTPUT_DIR)):
            if name.endswith(".json"):
                ts = int(name[:-5])
                pcd = np.loadtxt(os.path.join(G.OUTPUT_DIR, f"{ts}.pcd"), skiprows=10, ndmin=2)
                written[ts] = (json.load(open(os.path.join(G.OUTPUT_DIR, name))), pcd)
        # the writer's bytes for one small scene
        w_res_ts = frames[1]["ts"]
        fr0 = written[w_res_ts]
        w_points = np.column_stack([rng.uniform(-25, 25, (30, 3)), rng.uniform(-3, 260, 30)])
        w_items = fr0[0]["items"][:2]
        G.save_pcd(os.path.join(tmp, "w.pcd"), w_points)
        G.save_json_vma_direct(os.path.join(tmp, "w.json"), w_items, pose_ts[2], w_res_ts)
        w_pcd, w_json = open(os.path.join(tmp, "w.pcd"), "rb").read(), open(os.path.join(tmp, "w.json"), "rb").read()
    assert [p["ts"] for p in tool_poses] == sorted(pose_ts)
    order = np.argsort(pose_ts)                    # the tool's pose order (sorted by integer timestamp)
    assert list(order) == list(range(n_pose))

    # ---- what the tool wrote, frame by frame
    frames.sort(key=lambda fr: fr["ts"])
    expect_written = [fr for fr in frames if fr["pose"] >= 0 and fr["pose"] not in (ISLANDS["crop"], ISLANDS["disc"])
                      and any(len(px) > 1 for px in fr["pixels"])]
    assert sorted(written) == [fr["ts"] for fr in expect_written], (sorted(written), [fr["ts"] for fr in expect_written])
    out = {}
    sl_pts, sl_src, sl_off = [], [], [0]
    ctx_verts, ctx_len, ctx_lane, ctx_off = [], [], [], [0]
    match_all, match_off, cost_all, cost_shape = [], [0], [], []
    half = G.SEGMENT_LEN / 2
    for fr in expect_written:
        doc, pcd = written[fr["ts"]]
        j = fr["pose"]
        assert doc["timestamp"] == str(pose_ts[j]) and doc["result_timestamp"] == str(fr["ts"])
        pd = pose_dict(poses[j])
        # slice: membership from the intensity column, fp64 coordinates from transform_to_local
        src = pcd[:, 3].astype(np.int64)
        assert np.all(np.diff(src) > 0)
        loc = G.transform_to_local(cloud[src], pd)
        assert np.abs(loc - pcd[:, :3]).max() < 1e-4
        dx, dy = cloud[:, 0] - pd["x"], cloud[:, 1] - pd["y"]
        near = (dx ** 2 + dy ** 2) < 3600
        all_loc = G.transform_to_local(cloud[near], pd)
        assert np.abs(np.abs(all_loc[:, 0]) - half).min() > 1e-6, "a cloud point within 1e-6 m of a crop plane"
        assert np.array_equal(np.flatnonzero(near)[np.abs(all_loc[:, 0]) <= half], src)
        sl_pts.append(loc); sl_src.append(src); sl_off.append(sl_off[-1] + len(src))
        # context lines = the clipped GT of the frame, exact through JSON
        items = doc["items"]
        ctx = [np.array([[p["x"], p["y"], p["z"]] for p in l]) for l in items[0]["context_lines"]]
        assert len(ctx) == len(clipped[j]) and all(np.array_equal(a, b) for a, (_, b) in zip(ctx, clipped[j]))
        for l, lane in enumerate(lanes):
            d = np.abs(np.abs(G.transform_to_local(lane, pd)[:, 0]) - half)
            if l == special_dx and j == 9:
                assert np.sort(d)[:2].min() >= 2e-7 and np.sort(d)[2] > 1e-6
            else:
                assert d.min() > 1e-6, "a GT vertex within 1e-6 m of a clip plane"
        ctx_verts += ctx; ctx_len += [len(c) for c in ctx]; ctx_lane += [l for l, _ in clipped[j]]
        ctx_off.append(ctx_off[-1] + len(ctx))
        # items: one per kept instance, in order
        kept = [k for k, px in enumerate(fr["pixels"]) if len(px) > 1]
        assert len(items) == len(kept)
        preds, match = [], []
        for it, k in zip(items, kept):
            assert it["category"] == "lane_line" and it["context_lines"] == items[0]["context_lines"]
            assert it["attributes"] == {"score": fr["scores"][k] if fr["scores"][k] is not None else 0.0}
            cand = np.array([[p["x"], p["y"], p["z"]] for p in it["noisy_candidates"][0]])
            ego = G.pixel_to_ego([[float(u), float(v)] for u, v in fr["pixels"][k]])
            assert np.array_equal(cand, np.array([[p["x"], p["y"], p["z"]] for p in ego]))
            preds.append(cand)
            hit = [g for g, l in enumerate(items[0]["context_lines"]) if l == it["position"]]
            if fr["ts"] == tie_ts:
                match.append(hit[0] if hit else -1)
            else:
                assert len(hit) <= 1 and (bool(hit) == bool(it["position"]))
                match.append(hit[0] if hit else -1)
        cost = tool_cost(preds, ctx)
        if len(ctx):
            r, c = linear_sum_assignment(cost)
            want = np.full(len(preds), -1)
            for a, b in zip(r, c):
                if cost[a, b] < 15.0:
                    want[a] = b
                assert abs(cost[a, b] - 15.0) > 1e-6, "a matched cost within 1e-6 of the threshold"
            if fr["ts"] != tie_ts:
                assert list(want) == match, (fr["ts"], want, match)
                best = cost[r, c].sum()
                for a, b in zip(r, c):                  # uniqueness by a margin
                    alt = cost.copy()
                    alt[a, b] = 1e6
                    r2, c2 = linear_sum_assignment(alt)
                    assert alt[r2, c2].sum() - best >= 1e-6, "the optimal assignment is not unique by 1e-6"
        else:
            assert match == [-1] * len(preds)
        match_all += match; match_off.append(match_off[-1] + len(match))
        cost_all.append(cost.reshape(-1)); cost_shape.append(cost.shape)
        print(f"frame {fr['ts']}: pose {j}, {len(src)} points, P {len(preds)} x G {len(ctx)}, match {match}")
    far_fr = [fr for fr in expect_written if fr["pose"] == 7][0]
    k = [fr["ts"] for fr in expect_written].index(far_fr["ts"])
    assert match_all[match_off[k] + 1] == -1 and cost_all[k].reshape(cost_shape[k])[1].min() > 15.0

    # ---- inputs
    out["poses"] = poses
    out["pose_ts"] = np.array(pose_ts, dtype=np.int64)
    out["pose_names"] = np.frombuffer(json.dumps(pose_names).encode(), dtype=np.uint8)
    out["cloud"] = cloud
    out["gt_json"] = np.frombuffer(json.dumps(gt_doc).encode(), dtype=np.uint8)
    out["gt_verts"] = np.concatenate(lanes)
    out["gt_len"] = np.array([len(l) for l in lanes], dtype=np.int64)
    out["results_json"] = np.frombuffer(results_bytes, dtype=np.uint8)
    out["frame_ts"] = np.array([fr["ts"] for fr in frames], dtype=np.int64)
    out["frame_pose"] = np.array([fr["pose"] for fr in frames], dtype=np.int64)
    kept_px = [[px for px in fr["pixels"] if len(px) > 1] for fr in frames]
    out["frame_n_pred"] = np.array([len(k) for k in kept_px], dtype=np.int64)
    out["pred_len"] = np.array([len(px) for k in kept_px for px in k], dtype=np.int64)
    out["pred_pixels"] = np.concatenate([px for k in kept_px for px in k])
    out["pred_scores"] = np.array([sc if sc is not None else 0.0 for fr in frames
                                   for px, sc in zip(fr["pixels"], fr["scores"]) if len(px) > 1])
    ego = G.pixel_to_ego([[float(u), float(v)] for u, v in out["pred_pixels"]])
    out["pred_ego"] = np.array([[p["x"], p["y"], p["z"]] for p in ego])
    # ---- the reference's outputs
    out["written_ts"] = np.array([fr["ts"] for fr in expect_written], dtype=np.int64)
    out["written_pose"] = np.array([fr["pose"] for fr in expect_written], dtype=np.int64)
    out["tie_ts"] = np.int64(tie_ts)
    out["slice_points"] = np.concatenate(sl_pts)
    out["slice_source"] = np.concatenate(sl_src)
    out["slice_offsets"] = np.array(sl_off, dtype=np.int64)
    out["ctx_verts"] = np.concatenate(ctx_verts)
    out["ctx_len"] = np.array(ctx_len, dtype=np.int64)
    out["ctx_lane"] = np.array(ctx_lane, dtype=np.int64)
    out["ctx_offsets"] = np.array(ctx_off, dtype=np.int64)
    out["match"] = np.array(match_all, dtype=np.int64)
    out["match_offsets"] = np.array(match_off, dtype=np.int64)
    out["costs"] = np.concatenate(cost_all)
    out["cost_shapes"] = np.array(cost_shape, dtype=np.int64).reshape(-1, 2)
    # every lane in every pose's frame: gate, count and vertices of clip_polyline_by_x
    counts = np.zeros((n_pose, len(lanes)), dtype=np.int64)
    verts = []
    for s, p in enumerate(poses):
        for l, lane in enumerate(lanes):
            loc = G.transform_to_local(lane, pose_dict(p))
            if np.any((loc[:, 0] > -half) & (loc[:, 0] < half)):
                c = np.asarray(G.clip_polyline_by_x(loc, -half, half), dtype=np.float64).reshape(-1, 3)
                counts[s, l] = len(c)
                verts.append(c)
    out["clip_counts"] = counts
    out["clip_verts"] = np.concatenate(verts)
    out["special_dx_lane"] = np.int64(special_dx)
    # the writer
    out["w_points"] = w_points
    out["w_items"] = np.frombuffer(json.dumps(w_items).encode(), dtype=np.uint8)
    out["w_ts"] = np.array([pose_ts[2], w_res_ts], dtype=np.int64)
    out["w_pcd_bytes"] = np.frombuffer(w_pcd, dtype=np.uint8)
    out["w_json_bytes"] = np.frombuffer(w_json, dtype=np.uint8)

    buf = io.BytesIO()
    np.savez_compressed(buf, **out)
    assert buf.tell() <= 512 * 1024, buf.tell()
    with open(OUT, "wb") as f:
        f.write(buf.getvalue())
    print(f"wrote {OUT} ({buf.tell()} bytes)")


if __name__ == "__main__":
    main()
