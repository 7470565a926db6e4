"""Ground lift on the GPU (csrc/prh_ground.hpp through pointnet_refine_amd.ground) against the
restatement of the rule in _ground_oracle.py.  Every output array - height, count, hits, bin - is
compared with the oracle as bits: the rule's sums are integers, so there is nothing to tolerate.  The
designed cases come from the fixture g18 (stored inputs, stored results); the seeded ones from
_ground_cases.py, whose oracle results are computed once per process.  Then the gap itself, end to
end: a detector drive whose poses ride 1.7 m above the road with 0.02 rad of pitch.

The two end-to-end bounds: fused y within 1e-4 of the lanes (test_link_gpu's bound: the head is zero,
fp32 ulp at 100 m is 7.6e-6 and the path rounds a handful of times) and fused world z within 0.05 m
of the road at z = 0 (the cloud's noise is N(0, 0.02) and a station's height is a mean over tens of
points; 0.05 m is the bound test_ground_cpu derives for the analytic road)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import _fuse_oracle as FO
import _ground_cases as C
from pointnet_refine_amd import fuse as F
from pointnet_refine_amd import ground as GR
from pointnet_refine_amd import link as LK
from pointnet_refine_amd import predictions as PR

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _run(c, points=None, **more):
    res = GR.ground_heights(c["points"] if points is None else points, c["slice_offsets"], c["queries"], c["query_offsets"],
                            **dict(c["kw"], **more))
    assert all(res[k].is_cuda for k in C.KEYS)
    return {k: res[k].cpu().numpy() for k in C.KEYS}


def _same_bits(got, want, what):
    for k in C.KEYS:
        assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape, (what, k)
        bad = np.flatnonzero(C.bits(got[k]) != C.bits(want[k]))
        assert len(bad) == 0, (what, k, bad[:8], got[k][bad[:8]], want[k][bad[:8]])


@pytest.mark.parametrize("name", C.FIXTURE_CASES)
def test_fixture_cases_as_bits(golden_dir, name):
    """hits: 0, min_points - 1 and min_points hits, d2 == r2, non-finite points; bins: edges, just
    outside, bin 0, the last bin, equal modes, a climb of two, half-way qz; params: other parameters;
    cells: border points, 1 / 63 / 64 / 65 / 257 points in one cell - at cell = radius and 4 radius."""
    g = np.load(os.path.join(golden_dir, "g18_ground_lift.npz"))
    c = C.case(name)
    assert np.array_equal(C.bits(g[f"{name}_points"]), C.bits(c["points"][:, :3]))
    want = {k: g[f"{name}_{k}"] for k in C.KEYS}
    radius = c["kw"].get("radius", C.RADIUS)
    _same_bits(_run(c), want, name)
    _same_bits(_run(c, cell=radius), want, name + " cell = radius")
    _same_bits(_run(c, cell=4.0 * radius), want, name + " cell = 4 radius")
    _same_bits(_run(c, cell=1.3 * radius), want, name + " cell = 1.3 radius")


@pytest.mark.parametrize("n_q", [1, 4, 5, 64, 65])
def test_query_counts_as_bits(n_q):
    name = f"queries{n_q}"
    got = _run(C.case(name))
    _same_bits(got, C.expected(name), name)
    assert n_q == 1 or (got["hits"][-1] == 0 and got["bin"][-1] == -1)       # the query outside the points' extent


def test_ragged_slices_order_and_dtype():
    """Six slices (three roads that are each other's decoys, an empty slice, queries without points,
    points without queries); the points of every slice shuffled; float32 points of equal value."""
    c = C.case("ragged")
    want = C.expected("ragged")
    _same_bits(_run(c), want, "ragged")
    _same_bits(_run(c, cell=2.0), want, "ragged cell = 2")
    rng = np.random.default_rng(5)
    shuffled = c["points"].copy()
    so = c["slice_offsets"]
    for s in range(len(so) - 1):
        shuffled[so[s]:so[s + 1]] = shuffled[so[s]:so[s + 1]][rng.permutation(so[s + 1] - so[s])]
    _same_bits(_run(c, points=shuffled), want, "shuffled")
    f32 = c["points"].astype(np.float32)
    assert np.array_equal(f32.astype(np.float64)[:, :3], c["points"][:, :3])   # the case's coordinates are float32 values
    _same_bits(_run(c, points=f32), want, "float32")
    _same_bits(_run(c, points=torch.from_numpy(f32).cuda()), want, "float32 on the device")
    _same_bits(_run(c, points=torch.from_numpy(c["points"]).cuda()), want, "float64 on the device")
    # one slice alone (S = 1) is its part of the ragged result
    one = {"points": c["points"][so[1]:so[2]], "slice_offsets": np.array([0, so[2] - so[1]]), "kw": {},
           "queries": c["queries"][c["query_offsets"][1]:c["query_offsets"][2]],
           "query_offsets": np.array([0, c["query_offsets"][2] - c["query_offsets"][1]])}
    part = {k: want[k][c["query_offsets"][1]:c["query_offsets"][2]] for k in C.KEYS}
    _same_bits(_run(one), part, "S = 1")


def test_empty_inputs_and_validation():
    z = GR.ground_heights(np.zeros((0, 4)), [0], np.zeros((0, 2)), [0])
    assert all(z[k].shape == (0,) for k in C.KEYS)
    z = GR.ground_heights(np.zeros((0, 4)), [0, 0], np.array([[1.0, 2.0]]), [0, 1])
    assert np.isnan(z["height"].cpu().numpy()).all() and z["bin"].cpu().tolist() == [-1] and z["hits"].cpu().tolist() == [0]
    c = C.case("hits")
    for bad in ({"radius": 0.0}, {"radius": 4.5}, {"n_bins": 257}, {"min_points": 0}, {"cell": 0.25}, {"peak_share": (3, 2)}):
        with pytest.raises(ValueError):
            _run(c, **bad)
    with pytest.raises(ValueError):
        GR.ground_heights(c["points"][:, :3], c["slice_offsets"], c["queries"], c["query_offsets"])
    with pytest.raises(ValueError):
        GR.ground_heights(c["points"], [0, 3], c["queries"], c["query_offsets"])
    with pytest.raises(ValueError):
        GR.ground_heights(c["points"], c["slice_offsets"], c["queries"] * np.nan, c["query_offsets"])
    with pytest.raises(ValueError):
        GR.ground_heights(c["points"].astype(np.float16), c["slice_offsets"], c["queries"], c["query_offsets"])


def test_lift_lines_is_stations_heights_and_the_host_rule():
    import _ground_oracle as O
    c = C.case("ragged")
    lines = [[np.array([[0.0, 0.25, 0.0], [8.0, 0.25, 0.0], [16.0, 0.0, 0.0]]), np.array([[40.0, 0.0, 0.0], [44.0, 0.0, 0.0]])],
             [np.array([[1.0, -0.25, 7.0], [15.0, 0.25, 7.0]])], [], [], [np.array([[1.0, 0.0, 0.0], [3.0, 0.0, 0.0]])], []]
    lifted, rep = GR.lift_lines(c["points"], c["slice_offsets"], lines)
    flat = [l for ls in lines for l in ls]
    xy, arc, off = O.line_stations(flat, 1.0)
    qoff = off[np.cumsum([0] + [len(ls) for ls in lines])]
    h = O.ground_heights(c["points"], c["slice_offsets"], xy, qoff)["height"]
    want, flags = O.lift(flat, arc, off, h)
    got = [l for ls in lifted for l in ls]
    assert [len(ls) for ls in lifted] == [len(ls) for ls in lines]
    for a, b, src in zip(got, want, flat):
        assert np.array_equal(C.bits(a), C.bits(b)) and np.array_equal(a[:, :2], src[:, :2])
    assert list(flags) == [True, False, True, False]        # off the cloud and in the slice without points: unchanged
    assert rep == {"lines": 4, "lines_lifted": 2, "lines_unlifted": 2, "stations": int(len(arc)),
                   "stations_without_ground": int(np.isnan(h).sum())}
    assert np.abs(got[0][:, 2] + 1.7).max() <= 0.05 and np.abs(got[2][:, 2] + 0.4).max() <= 0.05 and got[1][0, 2] == 0.0


# ------------------------------------------------------------------ a detector run above the road
LANE_Y = (-1.7, 1.9)
POSE_Z, PITCH = 1.7, 0.02


def _write_raised_drive(root):
    """test_link_gpu's detector drive with the world road at z = 0 and the poses 1.7 m above it,
    pitched by 0.02 rad: 4 poses 25 m apart with a little yaw, a ground cloud of 60 k points under
    every line (x up to 128 m), and a
    results JSON whose pixels are two straight lanes as each frame's BEV sees them (ego |x| <= 24)."""
    from pointnet_refine_amd.pcd import write_pcd_host
    rng = np.random.default_rng(7)
    drive = root / "drive"
    (drive / "pose").mkdir(parents=True)
    n = 60000
    cloud = np.column_stack([rng.uniform(-8.0, 128.0, n), rng.uniform(-4.0, 4.0, n), rng.normal(0.0, 0.02, n),
                             rng.uniform(0.0, 60.0, n)])
    write_pcd_host(str(drive / "merged.pcd"), cloud)
    results = {}
    for k in range(4):
        ts = 1000 + k
        pose = np.array([25.0 * (k + 1), 0.3 * k, POSE_Z, *FO.quat_yaw_pitch(0.04 * (k - 1.5), PITCH)])
        json.dump({"ts": str(ts), "x": pose[0], "y": pose[1], "z": pose[2], "qx": pose[3], "qy": pose[4], "qz": pose[5],
                   "qw": pose[6]}, open(drive / "pose" / f"{ts}.json", "w"))
        inst = []
        for y in LANE_Y:
            lane = np.stack([np.linspace(-10.0, 140.0, 601), np.full(601, y), np.zeros(601)], 1)
            ego = FO.to_ego(lane, pose)
            ego = ego[np.abs(ego[:, 0]) <= 24.0][::20]
            pix = np.stack([(25.0 - ego[:, 1]) / 0.05, (25.0 - ego[:, 0]) / 0.05], 1)
            inst.append({"data": pix.tolist(), "score": 0.9})
        results[f"cam/{ts}.jpg"] = {"pred_instances": inst}
    json.dump(results, open(root / "results.json", "w"))
    F.write_map_json(str(root / "gt.json"), [[np.array([[-10.0, y, 0.0], [140.0, y, 0.0]])] for y in LANE_Y],
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


def test_refine_predictions_needs_the_lift_and_gets_it(tmp_path):
    drive = _write_raised_drive(tmp_path)
    model = _zero_head_model().cuda().eval()
    flat = LK.refine_predictions(model, str(drive), str(tmp_path / "results.json"))
    print(flat["report"])
    assert flat["report"]["pieces"] == 0 and flat["report"]["pieces_sparse"] == 8          # the gap
    assert not any(k.startswith("lift_") for k in flat["report"]) and flat["fused"] == []
    res = LK.refine_predictions(model, str(drive), str(tmp_path / "results.json"), lift=True)
    rep = res["report"]
    print(rep)
    assert rep["pieces"] == 8 and rep["pieces_sparse"] == 0 and rep["clusters_kept"] == 2 and len(res["fused"]) == 2
    assert rep["lift_lines"] == rep["lift_lines_lifted"] == 8 and rep["lift_lines_unlifted"] == 0
    # a line keeps every 20th of the lane's 0.25 m vertices inside |x| <= 24: it spans 40 to 48 m, 41 stations or more
    assert rep["lift_stations"] >= 8 * 41 and rep["lift_stations_without_ground"] == 0
    for parts in res["fused"]:
        assert len(parts) == 1 and len(parts[0]) > 200
        y = [abs(float(parts[0][:, 1].mean()) - v) for v in LANE_Y]
        print("fused: max |y - lane|", np.abs(parts[0][:, 1] - LANE_Y[int(np.argmin(y))]).max(), "max |z|",
              np.abs(parts[0][:, 2]).max())
        assert min(y) <= 1e-4 and np.abs(parts[0][:, 1] - LANE_Y[int(np.argmin(y))]).max() <= 1e-4
        assert np.abs(parts[0][:, 2]).max() <= 0.05
    bat = LK.refine_predictions(model, str(drive), str(tmp_path / "results.json"), lift=True, batched=True)
    assert bat["report"] == rep and bat["pieces"].tobytes() == res["pieces"].tobytes()
    assert len(bat["fused"]) == 2 and all(a.tobytes() == b.tobytes() for p, q in zip(bat["fused"], res["fused"])
                                          for a, b in zip(p, q))


def test_example_lifts(tmp_path):
    drive = _write_raised_drive(tmp_path)
    ckpt = tmp_path / "model.pth"
    torch.save(_zero_head_model().state_dict(), ckpt)
    out = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "refine_predictions.py"), str(drive),
                          str(tmp_path / "results.json"), "--checkpoint", str(ckpt), "--out", str(tmp_path / "map.json"),
                          "--lift"], capture_output=True, text=True, timeout=300)
    print(out.stdout[-2000:], out.stderr[-2000:])
    assert out.returncode == 0
    assert "GROUND LIFT  8 of 8 lines lifted" in out.stdout and "2 clusters" in out.stdout


def test_prediction_scenes_carry_the_lifted_z(tmp_path):
    from pointnet_refine_amd import drive as D
    drive = _write_raised_drive(tmp_path)
    args = (str(drive), str(tmp_path / "gt.json"), str(tmp_path / "results.json"))
    plain = PR.predictions_to_scenes(*args, str(tmp_path / "plain"), verbose=False)
    again = PR.predictions_to_scenes(*args, str(tmp_path / "again"), verbose=False, lift=False)
    lifted = PR.predictions_to_scenes(*args, str(tmp_path / "lifted"), verbose=False, lift=True)
    names = sorted(os.listdir(tmp_path / "plain"))
    assert len(names) == 8 and names == sorted(os.listdir(tmp_path / "again")) == sorted(os.listdir(tmp_path / "lifted"))
    for n in names:
        a, b = open(tmp_path / "plain" / n, "rb").read(), open(tmp_path / "again" / n, "rb").read()
        assert a == b, n                                    # lift=False: byte-identical files
        if n.endswith(".pcd"):
            assert a == open(tmp_path / "lifted" / n, "rb").read(), n
    assert "lift" not in plain and lifted["lift"]["lines_lifted"] == 8
    preds = [[PR.pixel_to_ego(px) for px in fr["pixels"]] for fr in PR.load_results(args[2])]
    own, _ = GR.lift_lines(lifted["points"], lifted["offsets"], preds)
    for f, ts in enumerate(lifted["frames"]):
        items = json.load(open(tmp_path / "lifted" / f"{ts}.json"))["items"]
        flat_items = json.load(open(tmp_path / "plain" / f"{ts}.json"))["items"]
        for i, it in enumerate(items):
            assert it["noisy_candidates"] == [D.xyz_dicts(own[f][i])]
            z = np.array([p["z"] for p in it["noisy_candidates"][0]])
            assert np.abs(z + POSE_Z).max() <= 1.0           # the road, 1.7 m below the pose and pitched over +-24 m
            assert all(p["z"] == 0.0 for p in flat_items[i]["noisy_candidates"][0])
            assert it["position"] == flat_items[i]["position"] and it["context_lines"] == flat_items[i]["context_lines"]
        assert np.array_equal(lifted["matches"][f], plain["matches"][f])
