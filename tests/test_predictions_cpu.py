"""Prediction scenes, host side: a numpy restatement of the reference tool's clip rule, cost
expression (tools/generate_inference_data_vma.py:265-315,400-402,434-448) and a plain-Python
shortest-augmenting-path assignment, pinned against the g12 fixture the reference's own main()
produced; the host functions of pointnet_refine_amd.predictions (pixels, the detector JSON, poses,
the nearest-pose rule, the writer's bytes); the frame generators the GPU tests use, with the share
of near-tie frames asserted here; and the GPU-only functions refusing to run without a GPU.  The
GPU tests (test_predictions_gpu.py) hold the HIP kernels to this restatement.

Tolerance: clipped vertices and costs within 1e-9 m absolute (fp64 rounding of these expressions
is about 1e-13; the scene files carry 1e-4); membership, counts, keep and match decisions exact."""
import json
import os

import numpy as np
import pytest
import torch

import test_drive_cpu as RD

TOL = 1e-9
HALF = 25.0
MAX_LINES = 128


def load_g12(golden_dir):
    return np.load(os.path.join(golden_dir, "g12_prediction_scenes.npz"))


def split(verts, lens):
    o = np.concatenate(([0], np.cumsum(lens))).astype(np.int64)
    return [verts[o[i]:o[i + 1]] for i in range(len(lens))]


# ------------------------------------------------------------------ the restatement
def clip_plane_ref(points, plane, is_max):
    """clip_polygon_against_plane (:265-300) on a list of (3,) arrays."""
    inside = (lambda p: p[0] <= plane) if is_max else (lambda p: p[0] >= plane)

    def cross(a, b):
        denom = b[0] - a[0]
        if abs(denom) < 1e-6:
            return a
        return a + ((plane - a[0]) / denom) * (b - a)

    out = []
    if len(points) and inside(points[0]):
        out.append(points[0])
    for a, b in zip(points[:-1], points[1:]):
        ia, ib = inside(a), inside(b)
        if ia and ib:
            out.append(b)
        elif ia != ib:
            out.append(cross(a, b))
            if ib:
                out.append(b)
    return out


def clip_frame_ref(local, half=HALF):
    """Gate (:400) + the two passes (:302-315): (k,3), k = 0 when no vertex is strictly inside."""
    local = np.asarray(local, dtype=np.float64).reshape(-1, 3)
    if not np.any((local[:, 0] > -half) & (local[:, 0] < half)):
        return np.empty((0, 3))
    out = clip_plane_ref(clip_plane_ref(list(local), -half, False), half, True)
    return np.array(out, dtype=np.float64).reshape(-1, 3)


def clip_lines_frames_ref(lines, poses, half=HALF):
    poses = np.asarray(poses, dtype=np.float64).reshape(-1, 7)
    out = [[clip_frame_ref(RD.to_local(l, p), half) if len(l) else np.empty((0, 3)) for l in lines] for p in poses]
    return np.array([[len(c) for c in row] for row in out], dtype=np.int64).reshape(len(poses), len(lines)), out


def cost_ref(pred_lines, gt_lines):
    """(P,G): mean over the prediction's vertices of the xy distance to the nearest GT vertex (:434-448)."""
    cost = np.zeros((len(pred_lines), len(gt_lines)))
    for i, p in enumerate(pred_lines):
        for j, g in enumerate(gt_lines):
            d = np.asarray(p)[:, None, :2] - np.asarray(g)[None, :, :2]
            cost[i, j] = np.sqrt((d * d).sum(2)).min(1).mean()
    return cost


def cost_frame_ref(pred_lines, gt_lines):
    """cost_ref for one frame in a few numpy calls: all prediction vertices against all GT vertices,
    the min per GT line and the mean per prediction by reduceat."""
    n_p, n_g = len(pred_lines), len(gt_lines)
    if n_p == 0 or n_g == 0:
        return np.zeros((n_p, n_g))
    p = np.concatenate([np.asarray(l, dtype=np.float64)[:, :2] for l in pred_lines])
    g = np.concatenate([np.asarray(l, dtype=np.float64)[:, :2] for l in gt_lines])
    p_len, g_len = np.array([len(l) for l in pred_lines]), np.array([len(l) for l in gt_lines])
    dx, dy = p[:, None, 0] - g[None, :, 0], p[:, None, 1] - g[None, :, 1]
    near = np.sqrt(np.minimum.reduceat(dx * dx + dy * dy, np.concatenate(([0], np.cumsum(g_len)[:-1])), axis=1))
    return np.add.reduceat(near, np.concatenate(([0], np.cumsum(p_len)[:-1])), axis=0) / p_len[:, None]


def costs_ref_threaded(frames, threads=16):
    from concurrent.futures import ThreadPoolExecutor
    with ThreadPoolExecutor(threads) as ex:
        return list(ex.map(lambda fr: cost_frame_ref(*fr), frames))


def _augment(a, u, v, col_row, i):
    """One shortest augmenting path from free row i (1-based) over the (nr,nc) matrix a; u, v, col_row
    (the row of each column, 0: free) are updated in place.  Column 0 is the virtual start."""
    nr, nc = a.shape
    col_row[0] = i
    minv = np.full(nc + 1, np.inf)
    used = np.zeros(nc + 1, dtype=bool)
    way = np.zeros(nc + 1, dtype=np.int64)
    j0 = 0
    for _ in range(nr + 1):                                   # bounded by the row count, as the kernel is
        used[j0] = True
        i0 = col_row[j0]
        cur = (a[i0 - 1] - u[i0]) - v[1:]
        free = ~used[1:]
        upd = free & (cur < minv[1:])
        minv[1:][upd] = cur[upd]
        way[1:][upd] = j0
        cand = np.where(free, minv[1:], np.inf)
        j1 = int(np.argmin(cand)) + 1                         # the lowest column on a tie
        delta = cand[j1 - 1]
        u[col_row[used]] += delta                             # the rows of the visited columns are distinct
        v[used] -= delta
        minv[~used] -= delta
        j0 = j1
        if col_row[j0] == 0:
            break
    while j0:
        j1 = way[j0]
        col_row[j0] = col_row[j1]
        j0 = j1


def _solve(a):
    nr, nc = a.shape
    u, v, col_row = np.zeros(nr + 1), np.zeros(nc + 1), np.zeros(nc + 1, dtype=np.int64)
    for i in range(1, nr + 1):
        _augment(a, u, v, col_row, i)
    return u, v, col_row


def _total(a, col_row):
    j = np.flatnonzero(col_row[1:] > 0)
    return float(sum(a[col_row[j + 1] - 1, j]))               # column order, one addition at a time


def assign_ref(cost, return_state=False):
    """Minimum-cost assignment of a (P,G) matrix by shortest augmenting paths with potentials (the
    classic O(n^3) form, the column scan in numpy), transposed when P > G so rows <= columns.
    Returns (match (P,) GT column or -1, total)."""
    cost = np.asarray(cost, dtype=np.float64)
    n_p, n_g = cost.shape
    if n_p == 0 or n_g == 0:
        return np.full(n_p, -1, dtype=np.int64), 0.0
    a = np.ascontiguousarray(cost.T if n_p > n_g else cost)
    u, v, col_row = _solve(a)
    match = np.full(n_p, -1, dtype=np.int64)
    j = np.flatnonzero(col_row[1:] > 0)
    if n_p > n_g:
        match[j] = col_row[j + 1] - 1
    else:
        match[col_row[j + 1] - 1] = j
    total = _total(a, col_row)
    return (match, total, (a, u, v, col_row)) if return_state else (match, total)


def unique_by(cost, margin=1e-6):
    """True when forbidding any pair of the optimal assignment raises the optimum by >= margin.  A
    forbidden pair is re-solved by one augmentation from the optimal potentials, which stay
    feasible when a cost goes up."""
    cost = np.asarray(cost, dtype=np.float64)
    if cost.size == 0:
        return True
    _, total, (a, u, v, col_row) = assign_ref(cost, return_state=True)
    for j in np.flatnonzero(col_row[1:] > 0) + 1:
        a2, u2, v2, cr2 = a.copy(), u.copy(), v.copy(), col_row.copy()
        i = cr2[j]
        a2[i - 1, j - 1] = 1e6
        cr2[j] = 0
        _augment(a2, u2, v2, cr2, i)
        if _total(a2, cr2) - total < margin:
            return False
    return True


def match_ref(pred_lines, gt_lines, threshold=15.0):
    cost = cost_ref(pred_lines, gt_lines)
    match, total = assign_ref(cost)
    for i in np.flatnonzero(match >= 0):
        if not cost[i, match[i]] < threshold:
            match[i] = -1
    return match, cost, total


# ------------------------------------------------------------------ generators (shared with the GPU tests)
def random_line(rng, n):
    a, b = rng.uniform(-25, 25, 2), rng.uniform(-25, 25, 2)
    return np.column_stack([a + np.linspace(0, 1, n)[:, None] * (b - a) + rng.normal(0, 0.3, (n, 2)), np.zeros(n)])


N_FRAMES, FRAMES_SEED = 2000, 31          # the at-size case of the GPU tests; its near-tie share is asserted here


def random_frames(n_frames=N_FRAMES, seed=FRAMES_SEED, max_side=MAX_LINES, max_verts=300):
    """[(pred lines, GT lines)]: P and G in 0..max_side (skewed to the small frames real drives have,
    mean about a third of max_side), the first frames forced through 0, 1, 63, 64, 65 and max_side
    on either side; vertex counts 2..max_verts (skewed: median 6, mean about 45, the first lines of
    the third frame forced to 2 and max_verts); every coordinate a continuous draw."""
    rng = np.random.default_rng(seed)
    edge = [0, 1, 63, 64, 65, max_side]
    forced = [(p, g) for p in edge for g in (1, 64, max_side)] + [(p, g) for g in edge for p in (1, 65, max_side)]
    frames = []
    for f in range(n_frames):
        n_p, n_g = forced[f] if f < len(forced) else (int((max_side + 1) * rng.uniform() ** 2),
                                                      int((max_side + 1) * rng.uniform() ** 2))
        nv = lambda: 2 + int((max_verts - 1) * rng.uniform() ** 6)
        frames.append(([random_line(rng, nv()) for _ in range(n_p)], [random_line(rng, nv()) for _ in range(n_g)]))
    if n_frames > 5:                       # frame 5 is 1 x max_side, frame 4 is 1 x 64
        frames[5][0][0], frames[5][1][0], frames[5][1][1] = random_line(rng, max_verts), random_line(rng, 2), \
            random_line(rng, max_verts)
        frames[4][0][0] = random_line(rng, 2)
    return frames


def lane_frame(rng, variant):
    """Parallel GT lanes 3.5 m apart with a vertex every 0.5 m; a prediction is a stretch of a lane
    shifted by <= 0.4 m and jittered.  variant 0: at most one prediction per lane, some lanes
    without (P <= G).  variant 1: every lane has one or two predictions, plus clutter lines across
    the lanes (P >= G).  Either way a lane's own prediction costs <= 0.6 and any other line >= 0.8,
    so the only prediction drawn from a lane must get that lane.  Returns (preds, gts, source lane
    of each prediction or -1)."""
    n_lanes = int(rng.integers(2, 9))
    yaw = rng.uniform(-0.3, 0.3)
    rot = np.array([[np.cos(yaw), -np.sin(yaw)], [np.sin(yaw), np.cos(yaw)]])
    gts = []
    for k in range(n_lanes):
        x = np.arange(-25.0, 25.01, 0.5) + rng.uniform(-0.05, 0.05, 101)
        y = 3.5 * (k - (n_lanes - 1) / 2) + 0.002 * x * x
        gts.append(np.column_stack([np.column_stack([x, y]) @ rot.T, rng.normal(0, 0.02, len(x))]))
    preds, src = [], []
    for k in range(n_lanes):
        for _ in range(int(rng.choice([0, 1, 1, 1]) if variant == 0 else rng.choice([1, 1, 2]))):
            g = gts[k]
            m = int(rng.integers(8, 40))
            t = np.sort(rng.uniform(0, len(g) - 1, m))
            i = np.minimum(t.astype(int), len(g) - 2)
            xy = g[i, :2] + (t - i)[:, None] * (g[i + 1, :2] - g[i, :2])
            ang = rng.uniform(0, 2 * np.pi)
            xy = xy + rng.uniform(0, 0.4) * np.array([np.cos(ang), np.sin(ang)]) + rng.normal(0, 0.03, (m, 2))
            preds.append(np.column_stack([xy, np.zeros(m)]))
            src.append(k)
    for _ in range(int(rng.integers(0, 4)) if variant == 1 else 0):       # across the lanes, 14 m or more
        m = int(rng.integers(15, 40))
        x0, y0 = rng.uniform(-20, 20), rng.uniform(-3.5, 3.5)
        xy = np.column_stack([x0 + rng.normal(0, 0.1, m), y0 + np.linspace(-7, 7, m) * rng.uniform(1, 1.5)])
        preds.append(np.column_stack([xy @ rot.T, np.zeros(m)]))
        src.append(-1)
    order = rng.permutation(len(preds))
    return [preds[i] for i in order], gts, [src[i] for i in order]


N_LANE_FRAMES, LANE_SEED = 300, 23


def lane_frames(n_frames=N_LANE_FRAMES, seed=LANE_SEED):
    rng = np.random.default_rng(seed)
    return [lane_frame(rng, f % 2) for f in range(n_frames)]


def assert_sole_predictions_matched(match, src):
    for i, k in enumerate(src):
        if k >= 0 and src.count(k) == 1:
            assert match[i] == k, (i, k, match, src)


def check_certificate(cost, match, total, u, v):
    """The optimality certificate of an assignment with potentials: dual feasibility, tightness on the
    matched pairs, a perfect matching of the smaller side, the total."""
    n_p, n_g = cost.shape
    eps = 1e-9 * max(1.0, float(np.abs(cost).max()) if cost.size else 1.0)
    if n_p == 0 or n_g == 0:
        assert np.all(match == -1) and total == 0.0
        return
    red = cost - u[:, None] - v[None, :]
    assert red.min() >= -eps, red.min()
    rows = np.flatnonzero(match >= 0)
    assert len(rows) == min(n_p, n_g)
    assert len(set(match[rows].tolist())) == len(rows) and match[rows].max() < n_g
    assert np.abs(red[rows, match[rows]]).max() <= eps
    assert abs(total - cost[rows, match[rows]].sum()) <= eps * len(rows)


# ------------------------------------------------------------------ the restatement against g12
def test_clip_rule_matches_reference(golden_dir):
    z = load_g12(golden_dir)
    lanes = split(z["gt_verts"], z["gt_len"])
    counts, out = clip_lines_frames_ref(lanes, z["poses"])
    assert np.array_equal(counts, z["clip_counts"])
    got = np.concatenate([c for row in out for c in row if len(c)])
    assert got.shape == z["clip_verts"].shape and np.abs(got - z["clip_verts"]).max() < TOL
    # the designed cases: the slab-crossing line is dropped where it was placed, the |dx| < 1e-6 one kept
    assert counts[3, 5] == 0 and RD.clip_ref(RD.to_local(lanes[5], z["poses"][3])).shape[0] == 2
    assert counts[9, int(z["special_dx_lane"])] >= 2


def test_context_lines_of_written_frames(golden_dir):
    z = load_g12(golden_dir)
    lanes = split(z["gt_verts"], z["gt_len"])
    ctx = split(z["ctx_verts"], z["ctx_len"])
    for k, j in enumerate(z["written_pose"]):
        counts, out = clip_lines_frames_ref(lanes, z["poses"][j:j + 1])
        keep = [l for l in range(len(lanes)) if counts[0, l] > 1]
        a, b = z["ctx_offsets"][k], z["ctx_offsets"][k + 1]
        assert keep == z["ctx_lane"][a:b].tolist()
        for l, want in zip(keep, ctx[a:b]):
            assert out[0][l].shape == want.shape and np.abs(out[0][l] - want).max() < TOL


def _frames_of(z):
    """Per written frame: (prediction lines (ego), context lines, match, cost matrix)."""
    ctx = split(z["ctx_verts"], z["ctx_len"])
    pred = split(z["pred_ego"], z["pred_len"])
    p_off = np.concatenate(([0], np.cumsum(z["frame_n_pred"])))
    frame_of = {int(ts): n for n, ts in enumerate(z["frame_ts"])}
    c_off = np.concatenate(([0], np.cumsum(z["cost_shapes"][:, 0] * z["cost_shapes"][:, 1])))
    out = []
    for k, ts in enumerate(z["written_ts"]):
        n = frame_of[int(ts)]
        out.append((pred[p_off[n]:p_off[n + 1]], ctx[z["ctx_offsets"][k]:z["ctx_offsets"][k + 1]],
                    z["match"][z["match_offsets"][k]:z["match_offsets"][k + 1]],
                    z["costs"][c_off[k]:c_off[k + 1]].reshape(z["cost_shapes"][k])))
    return out


def test_costs_and_assignment_match_reference(golden_dir):
    z = load_g12(golden_dir)
    shapes = set()
    for ts, (preds, ctx, want, cost) in zip(z["written_ts"], _frames_of(z)):
        match, got, total = match_ref(preds, ctx)
        assert got.shape == cost.shape
        if cost.size:
            assert np.abs(got - cost).max() < TOL
        if int(ts) == int(z["tie_ts"]):                     # two identical GT lines: any optimum is right
            m2, t2 = assign_ref(cost)
            rows = np.flatnonzero(m2 >= 0)
            assert len(rows) == min(cost.shape) and len(set(m2[rows].tolist())) == len(rows)
            assert abs(t2 - cost[np.arange(len(want)), want].sum()) < TOL
        else:
            assert match.tolist() == want.tolist()
            assert unique_by(cost)
        shapes.add((np.sign(cost.shape[0] - cost.shape[1]), min(cost.shape)))
    assert {(1, 5), (-1, 3), (0, 6), (0, 1), (1, 0)} <= shapes       # P > G, P < G, P = G, 1 x 1, G = 0


def test_assign_ref_against_brute_force():
    from itertools import permutations
    rng = np.random.default_rng(5)
    for n_p, n_g in ((1, 1), (2, 5), (5, 2), (4, 4), (6, 3), (3, 7)):
        cost = rng.uniform(0, 10, (n_p, n_g))
        match, total = assign_ref(cost)
        if n_p <= n_g:
            best = min(sum(cost[i, c[i]] for i in range(n_p)) for c in permutations(range(n_g), n_p))
        else:
            best = min(sum(cost[r[j], j] for j in range(n_g)) for r in permutations(range(n_p), n_g))
        assert abs(total - best) < 1e-12
        rows = np.flatnonzero(match >= 0)
        assert abs(cost[rows, match[rows]].sum() - best) < 1e-12 and len(rows) == min(n_p, n_g)


def test_fast_cost_restatement_is_the_plain_one(golden_dir):
    z = load_g12(golden_dir)
    for preds, ctx, _, cost in _frames_of(z):
        assert np.abs(cost_frame_ref(preds, ctx) - cost_ref(preds, ctx).reshape(cost.shape)).max(initial=0.0) < 1e-12
    for preds, gts in random_frames(40)[36:]:
        assert np.abs(cost_frame_ref(preds, gts) - cost_ref(preds, gts)).max(initial=0.0) < 1e-12


def test_generated_frames_stay_within_the_near_tie_cap():
    """The GPU test demands the restatement's matches exactly on every generated frame whose optimum
    is unique by >= 1e-6, and may leave out at most 1 % of the frames: the generators (same
    arguments as there) must stay inside that cap.  Also the sizes they promise."""
    frames = random_frames()
    sides = {len(p) for p, _ in frames} | {len(g) for _, g in frames}
    assert len(frames) >= 2000 and {0, 1, 63, 64, 65, MAX_LINES} <= sides and max(sides) == MAX_LINES
    verts = [len(l) for p, g in frames for l in p + g]
    assert min(verts) == 2 and max(verts) == 300
    left_out = sum(not unique_by(c) for c in costs_ref_threaded(frames))
    assert left_out <= 0.01 * len(frames), (left_out, len(frames))
    lanes = lane_frames()
    left_out = sum(not unique_by(cost_frame_ref(p, g)) for p, g, _ in lanes)
    assert left_out <= 0.01 * len(lanes), (left_out, len(lanes))


def test_lane_frames_match_their_source():
    for preds, gts, src in lane_frames():
        match, cost, _ = match_ref(preds, gts)
        own = [cost[i, k] for i, k in enumerate(src) if k >= 0]
        other = [cost[i, j] for i, k in enumerate(src) for j in range(len(gts)) if j != k]
        assert max(own, default=0.0) <= 0.6 and min(other, default=1.0) >= 0.8        # what the docstring promises
        assert_sole_predictions_matched(match, src)


# ------------------------------------------------------------------ the module's host functions
def test_pixel_to_ego(golden_dir):
    from pointnet_refine_amd import predictions as PR
    z = load_g12(golden_dir)
    got = PR.pixel_to_ego(z["pred_pixels"])
    assert got.dtype == np.float64 and np.array_equal(got, z["pred_ego"])
    assert np.array_equal(PR.pixel_to_ego([[0, 0], [1000, 1000], [500, 250]]),
                          np.array([[25.0, 25.0, 0.0], [-25.0, -25.0, 0.0], [12.5, 0.0, 0.0]]))
    assert PR.pixel_to_ego(np.zeros((0, 2))).shape == (0, 3)


def _write_drive(z, root):
    os.makedirs(os.path.join(root, "pose"), exist_ok=True)
    names = json.loads(bytes(z["pose_names"]).decode())
    for p, ts, name in zip(z["poses"], z["pose_ts"], names):
        with open(os.path.join(root, "pose", name + ".json"), "w") as f:
            json.dump({"ts": str(int(ts)), "x": float(p[0]), "y": float(p[1]), "z": float(p[2]), "qx": float(p[3]),
                       "qy": float(p[4]), "qz": float(p[5]), "qw": float(p[6])}, f)
    cloud = z["cloud"]
    rec = np.zeros(len(cloud), dtype=np.dtype([("x", "<f4"), ("y", "<f4"), ("z", "<f4"), ("i", "<u2")]))
    rec["x"], rec["y"], rec["z"], rec["i"] = cloud[:, 0], cloud[:, 1], cloud[:, 2], cloud[:, 3].astype(np.uint16)
    with open(os.path.join(root, "merged.pcd"), "wb") as f:
        f.write((f"VERSION 0.7\nFIELDS x y z intensity\nSIZE 4 4 4 2\nTYPE F F F U\nCOUNT 1 1 1 1\nWIDTH {len(cloud)}\n"
                 f"HEIGHT 1\nVIEWPOINT 0 0 0 1 0 0 0\nPOINTS {len(cloud)}\nDATA binary\n").encode())
        f.write(rec.tobytes())
    with open(os.path.join(root, "gt.json"), "wb") as f:
        f.write(bytes(z["gt_json"]))
    with open(os.path.join(root, "results.json"), "wb") as f:
        f.write(bytes(z["results_json"]))
    return root, os.path.join(root, "gt.json"), os.path.join(root, "results.json")


def test_load_results_and_poses(golden_dir, tmp_path):
    from pointnet_refine_amd import predictions as PR
    z = load_g12(golden_dir)
    root, _, results = _write_drive(z, str(tmp_path))
    frames = PR.load_results(results)
    assert [fr["ts"] for fr in frames] == z["frame_ts"].tolist()            # sorted; the odd key is ignored
    assert all(isinstance(fr["ts"], int) for fr in frames)
    assert [len(fr["pixels"]) for fr in frames] == z["frame_n_pred"].tolist()      # one-vertex instances dropped
    flat = [px for fr in frames for px in fr["pixels"]]
    assert [len(px) for px in flat] == z["pred_len"].tolist()
    assert np.array_equal(np.concatenate(flat), z["pred_pixels"])
    assert [s for fr in frames for s in fr["scores"]] == z["pred_scores"].tolist() and 0.0 in z["pred_scores"]
    poses = PR.load_frame_poses(os.path.join(root, "pose"))
    assert [p["ts"] for p in poses] == z["pose_ts"].tolist() and all(isinstance(p["ts"], int) for p in poses)
    from pointnet_refine_amd import drive
    assert np.array_equal(drive.poses_xyzq(poses), z["poses"])
    chosen = PR.match_poses([fr["ts"] for fr in frames], [p["ts"] for p in poses])
    assert chosen.tolist() == z["frame_pose"].tolist() and -1 in chosen


def test_match_poses_ties_limits_and_large_integers():
    from pointnet_refine_amd import predictions as PR
    t0 = 1_755_661_956_000_000_000
    assert float(t0 + 1) == float(t0)                               # float64 cannot tell these apart
    pose_ts = [t0, t0 + 100_000_000, t0 + 200_000_001]
    got = PR.match_poses([t0 + 50_000_000, t0 + 150_000_000, t0 + 150_000_001, t0 - 250_000_000, t0 - 250_000_001,
                          t0 + 450_000_001, t0 + 450_000_002], pose_ts)
    assert got.tolist() == [0, 1, 2, 0, -1, 2, -1]
    assert PR.match_poses([5], []).tolist() == [-1] and PR.match_poses([], [5]).shape == (0,)
    assert PR.match_poses([t0 + 3], [t0, t0 + 2, t0 + 4], max_gap=0).tolist() == [-1]
    assert PR.match_poses([t0 + 2], [t0, t0 + 2, t0 + 4], max_gap=0).tolist() == [1]


def test_writer_bytes(golden_dir, tmp_path):
    from pointnet_refine_amd import predictions as PR
    z = load_g12(golden_dir)
    items = json.loads(bytes(z["w_items"]).decode())
    pcd, js = str(tmp_path / "w.pcd"), str(tmp_path / "w.json")
    PR.write_prediction_scene(pcd, js, z["w_points"], items, int(z["w_ts"][0]), int(z["w_ts"][1]))
    assert open(pcd, "rb").read() == bytes(z["w_pcd_bytes"])
    assert open(js, "rb").read() == bytes(z["w_json_bytes"])
    from pointnet_refine_amd import io as IO
    back = IO.load_scene_items(js)
    assert len(back) == len(items) and all(len(it["noisy_candidates"]) == 1 for it in back)


def test_device_functions_need_a_gpu(monkeypatch):
    from pointnet_refine_amd import predictions as PR
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    line = np.zeros((2, 3))
    pose = np.array([[0, 0, 0, 0, 0, 0, 1.0]])
    for call in (lambda: PR.clip_lines_frames([line], pose),
                 lambda: PR.line_costs([line], [0, 1], [line], [0, 1]),
                 lambda: PR.assign(np.zeros(1), [0, 1], [[1, 1]]),
                 lambda: PR.match_predictions([[line]], [[line]]),
                 lambda: PR.predictions_to_scenes("nowhere", "gt.json", "results.json")):
        with pytest.raises(RuntimeError, match="GPU"):
            call()
