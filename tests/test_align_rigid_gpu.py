"""Rigid paint alignment on the GPU (prh_align_score_rigid and the cell-ordered select passes of
csrc/prh_align.hpp, through pointnet_refine_amd.align) against the restatement of the rule in
_align_rigid_oracle.py.  Both tables - score, hits - are compared with the oracle as bits: the rule's
sums are integers, so there is nothing to tolerate.  The designed cases come from the fixture g20
(stored inputs, stored results); the seeded ones from _align_rigid_cases.py, whose oracle results are
computed once per process.  Then the gap itself, end to end: a detector drive whose lines are turned
by 15 mrad about every ego origin and lie (0.3, 0.44) m from the paint.

The end-to-end bound is _align_rigid_cases.BOUND, the rule's step 9' at a line end 24 m out (0.0195 +
0.0324 + 0.012 = 0.0639 m), which the numpy restatement meets on the analytic frame in
test_align_rigid_cpu; every frame's pose equals the restatement's as bits.  Measured on the drive: the
fused map lies up to 0.499 m beside the lanes with the shift-only stages and within 0.017 m with the
rigid ones."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import _align_cases as C
import _align_rigid_cases as RC
import _align_rigid_oracle as RO
from pointnet_refine_amd import _lib as L
from pointnet_refine_amd import align as AL
from pointnet_refine_amd import fuse as F
from pointnet_refine_amd import link as LK
from pointnet_refine_amd import predictions as PR

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ORDERS = ("cell", "arrival")


def _run(c, points=None, **more):
    res = AL.rigid_scores(c["points"] if points is None else points, c["slice_offsets"], c["lines"], c["poses"],
                          c["pose_offsets"], c["pivots"], **dict(c["kw"], **more))
    assert sorted(res) == ["hits", "score"] and all(res[k].is_cuda and res[k].dtype == torch.int64 for k in RC.KEYS)
    return {k: res[k].cpu().numpy() for k in RC.KEYS}


def _same_bits(got, want, what):
    for k in RC.KEYS:
        assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape, (what, k)
        bad = np.flatnonzero(got[k] != want[k])
        assert len(bad) == 0, (what, k, bad[:8], got[k][bad[:8]], want[k][bad[:8]])


@pytest.mark.parametrize("name", RC.FIXTURE_CASES)
def test_fixture_cases_as_bits(golden_dir, name):
    """hits: d2 == r2 at theta = 0, the pairs one ulp apart on each side of the tube under a real
    rotation about a non-zero pivot, a zero-length segment, a line of one vertex, non-finite x y z I,
    qi == 0, a point in two tubes; tiles: 0 / 1 / 63 / 64 / 65 / 257 candidates under 16 / 1 / 15 / 16
    / 17 / 17 poses - in both orders, at cell 0.5, 1 and 4 m."""
    g = np.load(os.path.join(golden_dir, "g20_paint_align_rigid.npz"))
    c = RC.case(name)
    assert np.array_equal(C.bits(g[f"{name}_points"]), C.bits(c["points"]))
    assert np.array_equal(C.bits(g[f"{name}_vertices"]), C.bits(C.csr(c["lines"])[0]))
    assert np.array_equal(C.bits(g[f"{name}_table"]), C.bits(AL.pose_table(c["poses"])))
    want = {k: g[f"{name}_{k}"] for k in RC.KEYS}
    for order in ORDERS:
        _same_bits(_run(c, order=order), want, f"{name} {order}")
        for cell in (0.5, 1.0, 4.0):
            _same_bits(_run(c, cell=cell, order=order), want, f"{name} {order} cell = {cell}")


def test_segment_tiles_as_bits():
    """prh_align_tile() and prh_align_tile() + 1 segments in a slice, a line that straddles the tile."""
    assert L.lib().prh_align_tile() == C.TILE and L.lib().prh_align_max_poses() == AL.MAX_POSES
    for order in ORDERS:
        _same_bits(_run(RC.case("segtile"), order=order), RC.expected("segtile"), "segtile " + order)


def test_ragged_slices_order_and_dtype():
    """Six slices with non-zero pivots (an empty one, lines without points, points without lines, two
    tables); the points of every slice shuffled; float32 points of equal value; points on the
    device; cells of 0.5, 1 and 4 m; S = 1; order='cell' against order='arrival'."""
    c = RC.case("ragged")
    want = RC.expected("ragged")
    for cell in (0.5, 1.0, 4.0):
        by_cell, by_arrival = _run(c, cell=cell, order="cell"), _run(c, cell=cell, order="arrival")
        _same_bits(by_cell, want, f"ragged cell = {cell}")
        _same_bits(by_arrival, by_cell, f"ragged arrival against cell, cell = {cell}")
    rng = np.random.default_rng(5)
    shuffled = c["points"].copy()
    so = c["slice_offsets"]
    for s in range(len(so) - 1):
        shuffled[so[s]:so[s + 1]] = shuffled[so[s]:so[s + 1]][rng.permutation(so[s + 1] - so[s])]
    f32 = c["points"].astype(np.float32)
    assert np.array_equal(f32.astype(np.float64), c["points"])       # the case's values are float32 values
    for order in ORDERS:
        _same_bits(_run(c, points=shuffled, order=order), want, "shuffled " + order)
        _same_bits(_run(c, points=f32, order=order), want, "float32 " + order)
        _same_bits(_run(c, points=torch.from_numpy(f32).cuda(), order=order), want, "float32 on the device " + order)
        _same_bits(_run(c, points=torch.from_numpy(c["points"]).cuda(), order=order), want, "float64 on the device " + order)
        _same_bits(_run(c, intensity_floor=20.0, order=order), RC.expected("ragged", 20.0), "floor 20 " + order)
    ko = c["pose_offsets"]
    one = dict(c, points=c["points"][so[4]:so[5]], slice_offsets=np.array([0, so[5] - so[4]]), lines=[c["lines"][4]],
               poses=c["poses"][ko[4]:ko[5]], pose_offsets=np.array([0, ko[5] - ko[4]]), pivots=c["pivots"][4:5])
    for order in ORDERS:
        _same_bits(_run(one, order=order), {k: want[k][ko[4]:ko[5]] for k in RC.KEYS}, "S = 1 " + order)


def test_cell_order_sorts_the_records_and_keeps_them():
    """The cell passes leave every slice's records in ascending cell order, and they are the records
    the arrival passes leave."""
    c = RC.case("tiles")
    p = AL.prepare(*RC.args(c)[:5], AL.RADIUS, 0.0, 1.0, "test", pivots=c["pivots"], rigid=True)
    rec_c, off_c, host_c = AL.select_candidates(p, "cell")
    rec_a, off_a, host_a = AL.select_candidates(p)
    assert np.array_equal(host_c, host_a) and torch.equal(off_c, off_a) and np.diff(host_c).tolist() == [0, 1, 63, 64, 65, 257]
    rc, ra, m = rec_c.cpu().numpy(), rec_a.cpu().numpy(), p["maps"]
    for s in range(p["n_s"]):
        a, b = rc[host_c[s]:host_c[s + 1]], ra[host_c[s]:host_c[s + 1]]
        assert sorted(map(bytes, a)) == sorted(map(bytes, b))
        ix = np.floor((a[:, 0] - m["origin"][s, 0]) / m["cell"]).astype(np.int64)
        iy = np.floor((a[:, 1] - m["origin"][s, 1]) / m["cell"]).astype(np.int64)
        assert np.all(np.diff(iy * int(m["shape"][s, 0]) + ix) >= 0), s
    assert len({tuple(np.floor(r[:2])) for r in rc[host_c[5]:host_c[6]]}) > 4       # more than one cell in the big slice


@pytest.mark.parametrize("name", ["hits", "tiles", "ragged"])
def test_theta_zero_is_paint_scores(name):
    """An all-theta = 0 table with pivot (0, 0): AL.paint_scores' integers on the same inputs."""
    c = C.case(name)
    res = AL.paint_scores(c["points"], c["slice_offsets"], c["lines"], c["shifts"], c["shift_offsets"], **c["kw"])
    want = {k: res[k].cpu().numpy() for k in C.KEYS}
    _same_bits(want, C.expected(name), name + " paint_scores")
    poses = np.column_stack([c["shifts"], np.zeros(len(c["shifts"]))])
    for order in ORDERS:
        got = AL.rigid_scores(c["points"], c["slice_offsets"], c["lines"], poses, c["shift_offsets"], order=order, **c["kw"])
        _same_bits({k: got[k].cpu().numpy() for k in C.KEYS}, want, f"{name} {order}")


def test_empty_inputs_and_validation():
    z = AL.rigid_scores(np.zeros((0, 4)), [0], [], np.zeros((0, 3)), [0])
    assert all(z[k].shape == (0,) for k in RC.KEYS)
    line = [np.array([[0.0, 0.0, 0.0], [1.0, 0.0, 0.0]])]
    for order in ORDERS:
        z = AL.rigid_scores(np.zeros((0, 4)), [0, 0], [line], np.zeros((1, 3)), [0, 1], order=order)
        assert z["score"].cpu().tolist() == [0] and z["hits"].cpu().tolist() == [0]
        z = AL.rigid_scores(np.array([[0.5, 0.0, 0.0, 9.0]]), [0, 1], [line], np.zeros((0, 3)), [0, 0], order=order)
        assert z["score"].shape == (0,)
    c = RC.case("hits")
    for bad in ({"radius": 0.0}, {"radius": 1.5}, {"cell": 0.0}, {"intensity_floor": np.nan}, {"order": "sorted"}):
        with pytest.raises(ValueError):
            _run(c, **bad)
    a = RC.args(c)
    far = c["poses"].copy()
    far[0, 2] = 0.1000001                                       # |theta| > 0.1
    with pytest.raises(ValueError):
        AL.rigid_scores(*a[:3], far, *a[4:], radius=0.25)
    far[0, 2], far[0, 0] = 0.0, 4.5
    with pytest.raises(ValueError):
        AL.rigid_scores(*a[:3], far, *a[4:], radius=0.25)
    with pytest.raises(ValueError):
        AL.rigid_scores(*a[:3], c["poses"][:, :2], *a[4:])      # a (K,2) table
    with pytest.raises(ValueError):
        AL.rigid_scores(*a[:3], np.zeros((AL.MAX_POSES + 1, 3)), [0, 0, AL.MAX_POSES + 1], a[5])
    with pytest.raises(ValueError):
        AL.rigid_scores(*a[:4], [0, 3], a[5])
    for pivots in (c["pivots"][:1], c["pivots"].reshape(-1), np.zeros((2, 3)), [[np.nan, 0.0], [0.0, 0.0]], [[2e6, 0.0], [0.0, 0.0]]):
        with pytest.raises(ValueError):
            AL.rigid_scores(*a[:5], pivots)
    with pytest.raises(ValueError):
        AL.rigid_scores(c["points"][:, :3], *a[1:])
    with pytest.raises(RuntimeError):
        AL.rigid_scores(torch.from_numpy(c["points"]), *a[1:])  # a CPU tensor
    for bad in ({"scope": "lane"}, {"max_shift": 0.0}, {"max_yaw": -0.001}, {"max_yaw": 0.097}, {"lever": 0.0},
                {"keep": (65, 64)}, {"min_points": 0}, {"pivots": np.zeros((1, 2))}):
        with pytest.raises(ValueError):
            AL.align_lines_rigid(c["points"], c["slice_offsets"], c["lines"], **bad)
    # the library's own limits
    lib = L.lib()
    assert lib.prh_align_score_rigid(None, None, 0, None, 0, None, 0, None, None, None, 0, None, None, 0, None, 0, 2.0,
                                     None, 0, None) != 0
    assert "radius" in lib.prh_last_error().decode()
    assert lib.prh_align_score_rigid(None, None, 0, None, 0, None, 0, None, None, None, 0, None, None, 0, None, -1, 0.01,
                                     None, 0, None) != 0
    assert "align_score_rigid" in lib.prh_last_error().decode()
    assert lib.prh_align_select_cells_count(None, 1, None, 0, 0, None, None, None, None, 0, 0.0, 0.0, None, 0, None) != 0
    assert "cell" in lib.prh_last_error().decode()
    assert lib.prh_align_select_cells_write(None, 1, None, 0, 0, None, None, None, None, 0, 1.0, 0.0, None, None, -1, None, 0,
                                            0, None) != 0
    assert lib.prh_align_select_cells_workspace_bytes(1000) >= 4000 and lib.prh_align_select_cells_workspace_bytes(-1) == 0


def test_overflow_of_candidate_line_pairs():
    """2^20 candidates under 2^11 lines (all but one of a single vertex): 2^31 pairs in one slice."""
    n = 1 << 20
    pts = np.zeros((n, 4), dtype=np.float32)
    pts[:, 0] = np.linspace(0.0, 8.0, n, dtype=np.float32)
    pts[:, 3] = 30.0
    lines = [[np.array([[0.0, 0.0, 0.0], [8.0, 0.0, 0.0]])] + [np.array([[1.0, 1.0, 0.0]])] * ((1 << 11) - 1)]
    with pytest.raises(OverflowError):
        AL.rigid_scores(pts, [0, n], lines, np.zeros((1, 3)), [0, 1])


@pytest.mark.parametrize("scope", ["frame", "drive"])
def test_align_lines_rigid_is_two_stages_and_the_picks(scope):
    f = C.small_frames()
    lines = [[v.copy() for v in ls] for ls in f["lines"]]
    moved, rep = AL.align_lines_rigid(f["points"], f["slice_offsets"], lines, min_points=8, scope=scope)
    poses, aligned, zero, best = RC.small_align(scope)
    assert sorted(rep) == ["candidates", "frames", "frames_aligned", "frames_unaligned", "score_best", "score_zero", "shifts",
                           "yaws"]
    assert rep["shifts"].dtype == rep["yaws"].dtype == np.float64 and rep["yaws"].shape == (3,)
    assert np.array_equal(C.bits(rep["shifts"]), C.bits(np.ascontiguousarray(poses[:, :2])))
    assert np.array_equal(C.bits(rep["yaws"]), C.bits(np.ascontiguousarray(poses[:, 2])))
    assert rep["frames"] == 3 and rep["frames_aligned"] == sum(aligned) and rep["frames_unaligned"] == 3 - sum(aligned)
    assert rep["score_zero"].tolist() == zero and rep["score_best"].tolist() == best and rep["score_zero"].dtype == np.int64
    assert 48 <= rep["candidates"] <= len(f["points"])
    for s in range(3):
        for got, src in zip(moved[s], f["lines"][s]):
            want = np.array([RO.apply_pose(p, poses[s]) for p in src])
            assert np.array_equal(C.bits(got), C.bits(want)) and np.array_equal(got[:, 2], src[:, 2])
            assert np.array_equal(lines[s][0], src)             # the caller's lines are not written to


def test_max_yaw_zero_is_align_lines():
    f = C.small_frames()
    for scope in ("frame", "drive"):
        a, ra = AL.align_lines_rigid(f["points"], f["slice_offsets"], f["lines"], max_yaw=0.0, min_points=8, scope=scope)
        b, rb = AL.align_lines(f["points"], f["slice_offsets"], f["lines"], min_points=8, scope=scope)
        assert all(np.array_equal(C.bits(x), C.bits(y)) for p, q in zip(a, b) for x, y in zip(p, q))
        assert np.all(ra.pop("yaws") == 0.0) and sorted(ra) == sorted(rb)
        for k in rb:
            assert np.array_equal(ra[k], rb[k]) and np.asarray(ra[k]).dtype == np.asarray(rb[k]).dtype, k
    empty, rep0 = AL.align_lines_rigid(np.zeros((0, 4)), [0], [])
    assert empty == [] and rep0["frames"] == 0 and rep0["shifts"].shape == (0, 2) and rep0["yaws"].shape == (0,)
    assert rep0["candidates"] == 0


# ------------------------------------------------------------------ a detector run turned about the sensor
def _write_yawed_drive(root):
    """_align_rigid_cases.yawed_drive as files: merged.pcd, pose/*.json, a results JSON whose pixels
    are the two lanes turned by 15 mrad about each ego origin and moved by (0.3, 0.44) m, and the lanes as GT."""
    from pointnet_refine_amd.pcd import write_pcd_host
    cloud, poses, pixels = RC.yawed_drive()
    drive = root / "drive"
    (drive / "pose").mkdir(parents=True)
    write_pcd_host(str(drive / "merged.pcd"), cloud)
    results = {}
    for k, pose in enumerate(poses):
        ts = 1000 + k
        json.dump({"ts": str(ts), "x": pose[0], "y": pose[1], "z": pose[2], "qx": pose[3], "qy": pose[4], "qz": pose[5],
                   "qw": pose[6]}, open(drive / "pose" / f"{ts}.json", "w"))
        results[f"cam/{ts}.jpg"] = {"pred_instances": [{"data": px.tolist(), "score": 0.9} for px in pixels[k]]}
    json.dump(results, open(root / "results.json", "w"))
    F.write_map_json(str(root / "gt.json"), [[np.array([[-10.0, y, 0.0], [140.0, y, 0.0]])] for y in C.LANE_Y],
                     categories=["lane", "lane"])
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


def _worst_lane_error(fused):
    worst = 0.0
    for parts in fused:
        y = np.concatenate([p[:, 1] for p in parts])
        lane = C.LANE_Y[int(np.argmin([abs(float(y.mean()) - v) for v in C.LANE_Y]))]
        worst = max(worst, float(np.abs(y - lane).max()))
    return worst


def test_refine_predictions_needs_the_yaw_and_gets_it(tmp_path):
    drive = _write_yawed_drive(tmp_path)
    model = _zero_head_model().cuda().eval()
    args = (model, str(drive), str(tmp_path / "results.json"))
    shift_only = LK.refine_predictions(*args, align=True)
    left = _worst_lane_error(shift_only["fused"])
    print("align=True, shifts only: fused |y - lane| up to", left, shift_only["report"]["align_shifts"].tolist())
    assert "align_yaws" not in shift_only["report"] and left > 0.3       # the gap: a shift cannot take out the rotation
    res = LK.refine_predictions(*args, align=True, align_max_yaw=0.02)
    rep = res["report"]
    print({k: v for k, v in rep.items() if k.startswith("align_")})
    assert rep["align_frames"] == rep["align_frames_aligned"] == 4 and rep["align_yaws"].shape == (4,)
    assert rep["pieces"] == 8 and rep["clusters_kept"] == 2 and len(res["fused"]) == 2
    # the restatement over the very slices refine_predictions cut
    scenes = PR.predictions_to_scenes(str(drive), str(tmp_path / "gt.json"), str(tmp_path / "results.json"), verbose=False)
    preds = [[PR.pixel_to_ego(px) for px in fr["pixels"]] for fr in PR.load_results(str(tmp_path / "results.json"))]
    want, aligned, zero, best = RO.align(scenes["points"].cpu().numpy(), scenes["offsets"].cpu().numpy(), preds,
                                         scores=RC.rigid_scores_np)
    assert aligned == [True] * 4
    assert np.array_equal(C.bits(rep["align_shifts"]), C.bits(np.ascontiguousarray(want[:, :2])))
    assert np.array_equal(C.bits(rep["align_yaws"]), C.bits(np.ascontiguousarray(want[:, 2])))
    assert rep["align_score_zero"].tolist() == zero and rep["align_score_best"].tolist() == best
    worst = _worst_lane_error(res["fused"])
    print("align_max_yaw = 0.02: fused |y - lane| up to", worst, "bound", RC.BOUND)
    assert worst <= RC.BOUND
    both = LK.refine_predictions(*args, align=True, align_max_yaw=0.02, batched=True)
    ra, rb = dict(res["report"]), dict(both["report"])
    for k in ("align_shifts", "align_yaws", "align_score_zero", "align_score_best"):
        assert np.array_equal(C.bits(ra.pop(k)), C.bits(rb.pop(k))), k
    assert ra == rb and res["pieces"].tobytes() == both["pieces"].tobytes() and len(res["fused"]) == len(both["fused"])
    assert all(x.tobytes() == y.tobytes() for p, q in zip(res["fused"], both["fused"]) for x, y in zip(p, q))
    one = LK.refine_predictions(*args, align=True, align_max_yaw=0.02, align_scope="drive")
    sh, yw = one["report"]["align_shifts"], one["report"]["align_yaws"]
    assert sh.shape == (4, 2) and all(np.array_equal(C.bits(sh[0]), C.bits(sh[k])) and yw[0] == yw[k] for k in range(4))
    assert one["report"]["align_frames_aligned"] == 4 and _worst_lane_error(one["fused"]) <= RC.BOUND


def test_example_prints_the_yaw_only_when_asked(tmp_path):
    drive = _write_yawed_drive(tmp_path)
    ckpt = tmp_path / "model.pth"
    torch.save(_zero_head_model().state_dict(), ckpt)
    cmd = [sys.executable, os.path.join(ROOT, "examples", "refine_predictions.py"), str(drive), str(tmp_path / "results.json"),
           "--checkpoint", str(ckpt), "--out", str(tmp_path / "map.json"), "--align"]
    lines = {}
    for name, more in (("plain", []), ("yaw", ["--align-max-yaw", "0.02"])):
        out = subprocess.run(cmd + more, capture_output=True, text=True, timeout=300)
        print(out.stdout[-2000:], out.stderr[-2000:])
        assert out.returncode == 0
        lines[name] = [ln for ln in out.stdout.splitlines() if ln.startswith("PAINT ALIGN")]
    assert len(lines["plain"]) == len(lines["yaw"]) == 1
    assert "PAINT ALIGN  4 of 4 frames" in lines["yaw"][0] and "|yaw| median" in lines["yaw"][0] and "mrad" in lines["yaw"][0]
    assert "yaw" not in lines["plain"][0] and "|shift| median" in lines["plain"][0]


def test_prediction_scenes_carry_the_posed_xy(tmp_path):
    from pointnet_refine_amd import drive as D
    drive = _write_yawed_drive(tmp_path)
    args = (str(drive), str(tmp_path / "gt.json"), str(tmp_path / "results.json"))
    plain = PR.predictions_to_scenes(*args, str(tmp_path / "plain"), verbose=False)
    moved = PR.predictions_to_scenes(*args, str(tmp_path / "moved"), verbose=False, align=True, align_max_yaw=0.02)
    names = sorted(os.listdir(tmp_path / "plain"))
    assert len(names) == 8 and names == sorted(os.listdir(tmp_path / "moved"))
    for n in names:
        if n.endswith(".pcd"):
            assert open(tmp_path / "plain" / n, "rb").read() == open(tmp_path / "moved" / n, "rb").read(), n
    assert "align" not in plain and moved["align"]["frames_aligned"] == 4 and np.all(np.abs(moved["align"]["yaws"]) > 0.01)
    shifts, yaws = moved["align"]["shifts"], moved["align"]["yaws"]
    preds = [[PR.pixel_to_ego(px) for px in fr["pixels"]] for fr in PR.load_results(args[2])]
    for f, ts in enumerate(moved["frames"]):
        items = json.load(open(tmp_path / "moved" / f"{ts}.json"))["items"]
        plain_items = json.load(open(tmp_path / "plain" / f"{ts}.json"))["items"]
        assert len(items) == len(plain_items) == 2
        for i, it in enumerate(items):
            want = AL.apply_pose(preds[f][i], (shifts[f, 0], shifts[f, 1], yaws[f]))
            assert it["noisy_candidates"] == [D.xyz_dicts(want)]
            assert [p["z"] for p in it["noisy_candidates"][0]] == [p["z"] for p in plain_items[i]["noisy_candidates"][0]]
            assert {k: v for k, v in it.items() if k != "noisy_candidates"} == \
                {k: v for k, v in plain_items[i].items() if k != "noisy_candidates"}
        assert np.array_equal(moved["matches"][f], plain["matches"][f])
