"""Piece linking on the GPU (csrc/prh_link.hpp through pointnet_refine_amd.link) against the
restatement of the rule in _link_oracle.py: the stored fixture, seeded cases whose shapes are chosen
to break the kernels, degenerate pieces, reproducibility, fuse_unmatched end to end and
refine_predictions on a synthetic detector run.

Tolerances follow test_fuse_gpu.py.  pairs, n_in, n_out, edge, rho, cluster, sign, C and seg are
compared exactly; that is well-posed because every case asserts the margins the fixture's maker
asserts (each at least MARGIN = 1e-6: |d - gate| of interior points, the unclamped u of a point on
a polyline's first segment from 0 and on its last from 1 unless it is exactly 0 or 1 there - a
point that coincides with that end, exact on both sides -, the lead in d2 of a point's best segment
over the segments not next to it, the slack of every box comparison, |sum_dot| of edges, and for the
map the draft-carrier node margin and the two margins of test_fuse_gpu).  Sums, delta, offsets, g,
X, W and spread are compared to TOL = 1e-9 m, by the bound in test_fuse_gpu's docstring: device
coordinates are within 2.5 km of the origin (asserted), so an operation's rounding is at most
2.2e-16 * 2.5e3 and the at most 128 additions of a sum stay below 1e-10."""
import functools
import json
import os

import numpy as np
import pytest
import torch

import _fuse_oracle as O
import _link_oracle as K
from pointnet_refine_amd import fuse as F
from pointnet_refine_amd import link as LK

pytestmark = pytest.mark.gpu
TOL = 1e-9
MARGIN = 1e-6
BASE = np.array([400123.0, 3200456.0, 52.0])
ZERO = np.zeros(3)
INT_KEYS = ("pairs", "n_in", "n_out", "edge", "rho")
SUM_KEYS = ("sum_d", "sum_self", "sum_other", "sum_dot", "delta")


def _golden(golden_dir):
    return dict(np.load(os.path.join(golden_dir, "g16_piece_links.npz")))


def _assert_links(got, want):
    figures = {k: float(np.abs(got[k] - want[k]).max(initial=0.0)) for k in SUM_KEYS}
    print("candidates:", len(want["edge"]), "edges:", int(want["edge"].sum()), "max |gpu - oracle|:", figures)
    for k in INT_KEYS:
        assert got[k].shape == want[k].shape and np.array_equal(got[k], want[k]), k
    assert got["pairs"].dtype == np.int64 and got["n_in"].dtype == np.int32 and got["n_out"].dtype == np.int32
    assert got["edge"].dtype == bool
    for k, v in figures.items():
        assert v <= TOL, (k, v)


def _exact_ends(track):
    """The margins of a run, with the end margin taken over the points that do not sit exactly on
    the end (u exactly 0 or 1 there is exact on both sides)."""
    t = dict(track)
    t["end"] = [v for v in track["end"] if v != 0.0]
    return K.margins(t)


def _check(world, frame, gate=1.0, want=None):
    """link_pieces on shifted drive-frame pieces against the oracle: margins asserted, integers
    equal, the rest within TOL.  Returns (gpu, oracle)."""
    world = np.asarray(world, dtype=np.float64)
    assert np.abs(world).max(initial=0.0) < 2500.0
    if want is None:
        track = K.new_track()
        want = K.link(world, frame, gate, track=track)
        marg = _exact_ends(track)
        print("margins:", marg)
        assert min(marg.values()) >= MARGIN, marg
    got = LK.link_pieces(world, frame, gate=gate, origin=ZERO)
    _assert_links(got, want)
    return got, want


# ------------------------------------------------------------------ the fixture
def test_fixture_links(golden_dir):
    g = _golden(golden_dir)
    want = {k: g["link_" + k] for k in INT_KEYS + SUM_KEYS}
    _check(g["world_shifted"], g["piece_pose"], want=want)
    # from the drive frame proper, 400 km from zero: the default origin is the stored one
    got = LK.link_pieces(g["world_shifted"] + g["origin"], g["piece_pose"])
    _assert_links(got, want)


def _assert_map(n, fused, g):
    """fuse_unmatched's result against the stored steps 1-8 of the oracle."""
    for k in ("cluster", "sign", "kept"):
        assert np.array_equal(n[k], g[k]), k
    assert np.array_equal(n["clusters_all"], g["clusters_all"]) and np.array_equal(n["level"], g["level"])
    assert np.array_equal(n["parent"], g["parent"])
    assert np.array_equal(n["C"], g["map_C"]) and np.array_equal(n["seg"], g["map_seg"])
    assert np.array_equal(n["offsets"], g["map_offsets"]) and np.array_equal(n["origin"], g["origin"])
    figures = {k: float(np.abs(n[k] - g[k]).max()) for k in ("offset", "g")}
    figures.update({k: float(np.abs(n[k] - g["map_" + k]).max()) for k in ("world", "s", "d", "X", "W", "spread")})
    off = g["carrier_offsets"]
    assert [len(c) for c in n["carriers"]] == np.diff(off).tolist()
    figures["carriers"] = max(float(np.abs(c - g["carrier_vertices"][off[l]:off[l + 1]]).max())
                              for l, c in enumerate(n["carriers"]))
    print("max |gpu - oracle|:", figures)
    for k, v in figures.items():
        assert v <= TOL, (k, v)
    parts = np.split(g["fused_vertices"], np.cumsum(g["fused_sizes"])[:-1])
    want = [[p for p, l in zip(parts, g["fused_line"]) if l == c] for c in range(len(off) - 1)]
    assert len(fused) == len(want)
    for a, b in zip(fused, want):
        assert [len(x) for x in a] == [len(x) for x in b]
        assert all(np.abs(x - y).max() <= TOL for x, y in zip(a, b))


def test_fixture_map(golden_dir):
    """fuse_unmatched end to end on the fixture's case equals the oracle's steps 1-8 (stored; the
    maker asserted every margin, test_link_cpu restates the linking ones on the stored arrays)."""
    g = _golden(golden_dir)
    fused, n = LK.fuse_unmatched(g["pieces"], g["piece_pose"], g["poses"], step=float(g["step"]), return_nodes=True)
    _assert_links(n["links"], {k: g["link_" + k] for k in INT_KEYS + SUM_KEYS})
    _assert_map(n, fused, g)
    assert len(fused) == 4 and all(len(f) == 1 for f in fused)
    for c in range(4):                                 # pure and complete, as the oracle's clusters are
        assert len(np.unique(g["truth"][n["cluster"] == c])) == 1 and (n["cluster"] == c).sum() == 25
    assert LK.fuse_unmatched(g["pieces"][:0], g["piece_pose"][:0], g["poses"]) == []


def test_min_pieces_drops_a_lone_piece(golden_dir):
    g = _golden(golden_dir)
    lone = g["pieces"][:1] + [0.0, 40.0, 0.0]          # 40 m to the side of everything, seen once
    pieces, pose = np.concatenate([g["pieces"], lone]), np.append(g["piece_pose"], g["piece_pose"][0])
    fused, n = LK.fuse_unmatched(pieces, pose, g["poses"], step=float(g["step"]), return_nodes=True)
    assert n["cluster"][100] == -1 and n["clusters_all"][100] == 4 and len(fused) == 4
    assert np.array_equal(n["cluster"][:100], g["cluster"]) and np.array_equal(n["kept"], g["kept"])
    _assert_map({k: (v[:100] if k in ("cluster", "sign", "clusters_all", "level", "parent", "offset", "g") else v)
                 for k, v in n.items()}, fused, g)
    # kept with min_pieces = 1 it has no second view, and a draft carrier of its own
    fused1, n1 = LK.fuse_unmatched(pieces, pose, g["poses"], step=float(g["step"]), min_pieces=1, return_nodes=True)
    assert n1["cluster"][100] == 4 and len(fused1) == 5 and len(fused1[4]) == 1
    # every cluster too small: nothing is kept, and the answer still has its shape
    fused9, n9 = LK.fuse_unmatched(pieces, pose, g["poses"], min_pieces=26, return_nodes=True)
    assert fused9 == [] and (n9["cluster"] == -1).all() and len(n9["C"]) == 0 and n9["g"].shape == (101, 32)


# ------------------------------------------------------------------ shapes
@functools.lru_cache(maxsize=None)
def _lanes_case(m, seed):
    """Three lanes (two 3.5 m apart, one at 12 m) seen from 6 frames 10 m apart, in the shifted drive
    frame: 18 pieces of m points over 50 m windows (4 m for m = 2, where a piece is one segment and
    must stay within the gate of the curve), 3 cm noise, every fourth reversed, shuffled."""
    rng = np.random.default_rng(seed)
    half = 2.0 if m == 2 else 25.0
    step = 1.0 if m == 2 else 10.0
    world, frame = [], []
    for f in range(6):
        for lat in (-3.5, 0.0, 12.0):
            x = np.linspace(100.0 + step * f - half, 100.0 + step * f + half, m)
            world.append(K.lane_points(lat, x) + rng.normal(0.0, 0.03, (m, 3)) + [300.0, -700.0, 0.0])
            frame.append(f)
    world = np.stack(world)
    world[::4] = world[::4, ::-1]
    order = rng.permutation(len(world))
    return world[order], np.array(frame)[order]


@pytest.mark.parametrize("m", [2, 5, 32, 33, 64])
def test_points_per_piece(m):
    """M = 2: one segment, both first and last.  M = 32 fills both half-waves, M = 33 takes the first
    lane past them (the directions then run in turn), M = 64 fills the wave."""
    world, frame = _lanes_case(m, 200 + m)
    got, want = _check(world, frame)
    assert len(want["edge"]) >= 30 and (want["n_in"] > 0).sum() >= 20
    assert (want["rho"] == -1).any() and (want["rho"] == 1).any()
    if m > 2:                                          # two points cannot reach min_in = 4, and 4 m chords of
        assert want["edge"].sum() >= 20 and (~want["edge"]).any() and (want["n_out"] > 0).any()   # two lanes never meet
        assert LK.sync_pieces(len(world), got)["cluster"].max() == 2          # the three lanes


def _chain_case(n_pieces, seed):
    """n_pieces short pieces of 3 points along one line, 0.7 m apart, 7 frames in turn: every piece
    has candidates a few places up and down the list only, so rows end near the diagonal."""
    rng = np.random.default_rng(seed)
    world = np.zeros((n_pieces, 3, 3))
    for p in range(n_pieces):
        x = 0.7 * p + np.array([0.0, 1.4, 3.1])
        world[p] = np.stack([x, 0.05 * np.sin(x) + 5.0, np.zeros(3)], 1) + rng.normal(0.0, 0.02, (3, 3))
    return world, np.arange(n_pieces) % 7


@pytest.mark.parametrize("n_pieces", [1, 2, 64, 65, "tile+1"])
def test_piece_counts(n_pieces):
    """No pair, one row, the ballot word boundary and the LDS tile boundary of the pair kernels."""
    from pointnet_refine_amd import _lib
    lib = _lib.lib()
    if n_pieces == "tile+1":
        n_pieces = lib.prh_link_tile() + 1
    assert n_pieces <= 300
    world, frame = _chain_case(n_pieces, 300 + n_pieces)
    got, want = _check(world, frame)
    if n_pieces == 1:
        assert len(got["edge"]) == 0
    elif n_pieces == 2:
        assert got["pairs"].tolist() == [[0, 1]]
    else:
        assert len(got["edge"]) > 4 * n_pieces and got["pairs"][-1].tolist() == [n_pieces - 2, n_pieces - 1]
    if n_pieces > 64:
        assert len(got["edge"]) % lib.prh_link_pairs_per_block() != 0     # the last block of prh_link_stats is not full


def test_rows_longer_than_a_ballot_word():
    """130 two-point pieces across one another in a 6 m patch, 5 frames: rows of up to a hundred
    candidates, compacted over several 64-lane words and across the tile boundary."""
    rng = np.random.default_rng(77)
    a = rng.uniform(0.0, 6.28, 130)
    centre = rng.uniform(-1.0, 1.0, (130, 2))
    d = np.stack([np.cos(a), np.sin(a)], 1) * rng.uniform(2.0, 3.0, (130, 1))
    world = np.zeros((130, 2, 3))
    world[:, 0, :2], world[:, 1, :2] = centre - d, centre + d
    frame = np.arange(130) % 5
    got, want = _check(world, frame)
    assert np.bincount(want["pairs"][:, 0]).max() > 64 and len(want["edge"]) > 6000


# ------------------------------------------------------------------ degenerate pieces
def _straight(x0, x1, y, m=6, direction=(1.0, 0.0)):
    t = np.linspace(x0, x1, m)
    dx, dy = direction
    return np.stack([t * dx - y * dy, t * dy + y * dx, np.zeros(m)], 1)


def test_degenerate_pieces():
    diag = (np.sqrt(0.5), np.sqrt(0.5))                # along the diagonal, so parallel pieces share their boxes

    def line(t0, t1, side):
        return _straight(t0, t1, side, direction=diag)

    base = line(0.0, 10.0, 0.0)
    dup = line(1.0, 11.0, 0.3)
    dup[3] = dup[2]                                    # a zero-length segment inside
    point = np.repeat(line(5.1, 5.1, 1.4)[:1], 6, axis=0)                 # no usable segment at all
    twin = line(30.03, 40.0, 0.0) + [0.0, 0.0, 0.01]
    para_a, para_b = line(60.0, 70.0, 0.0), line(60.0, 70.0, 1.5)         # gate + 0.5 apart
    anti_a, anti_b = line(100.0, 110.0, 0.0), line(101.0, 111.0, 0.2)[::-1]
    world = np.stack([base, dup, point, twin, twin.copy(), para_a, para_b, anti_a, anti_b])
    frame = np.arange(len(world))
    got, want = _check(world, frame)
    stats = {tuple(p): k for k, p in enumerate(got["pairs"].tolist())}
    assert sorted(stats) == [(0, 1), (0, 2), (1, 2), (3, 4), (5, 6), (7, 8)]
    k = stats[(0, 1)]
    assert got["edge"][k] and got["rho"][k] == 1 and got["n_out"][k] == 0
    # the piece that is one point: its own six points are out (1.4 m and 1.1 m away), nothing counts on it
    for other in (0, 1):
        k = stats[(other, 2)]
        assert got["n_in"][k] == 0 and got["n_out"][k] == 6 and not got["edge"][k]
    # identical pieces: the four interior points of each at distance 0, the ends coincide with the other's ends
    k = stats[(3, 4)]
    assert got["n_in"][k] == 8 and got["n_out"][k] == 0 and got["sum_d"][k] <= 1e-12 and got["edge"][k]
    assert got["rho"][k] == 1 and abs(got["delta"][k]) <= 1e-12
    # gate + 0.5 apart: every interior point is out
    k = stats[(5, 6)]
    assert got["n_in"][k] == 0 and got["n_out"][k] >= 8 and not got["edge"][k] and got["delta"][k] == 0.0
    k = stats[(7, 8)]
    assert got["rho"][k] == -1 and got["edge"][k] and got["n_in"][k] >= 8
    s = LK.sync_pieces(len(world), got)
    assert s["sign"][8] == -1 and s["cluster"][8] == s["cluster"][7] and s["cluster"][5] != s["cluster"][6]
    assert abs(s["offset"][8] - 11.0) < 0.05           # anti_b starts 11 m along anti_a and runs back


def test_one_frame_and_no_pieces():
    world, _ = _lanes_case(5, 205)
    got = LK.link_pieces(world, np.zeros(len(world), dtype=np.int64), origin=ZERO)       # all in one frame
    assert got["pairs"].shape == (0, 2) and got["edge"].shape == (0,) and got["sum_d"].shape == (0,)
    got = LK.link_pieces(np.zeros((0, 5, 3)), np.zeros(0, dtype=np.int64))
    assert got["pairs"].shape == (0, 2) and got["n_in"].dtype == np.int32 and got["delta"].shape == (0,)
    s = LK.sync_pieces(0, got)
    assert len(s["cluster"]) == 0


def test_pair_outside_the_pieces_gives_nan():
    """The C ABI's promise for a pair list that names no piece: counts of -1, NaN sums, no fault."""
    from pointnet_refine_amd import _gpu as G
    from pointnet_refine_amd import _lib
    lib = _lib.lib()
    world, _ = _lanes_case(5, 205)
    dev = torch.device("cuda", torch.cuda.current_device())
    w = torch.from_numpy(world).to(dev)
    cum = torch.from_numpy(LK.piece_cums(world)).to(dev)
    offsets = torch.tensor([0, 3] + [3] * (len(world) - 1), dtype=torch.int64, device=dev)
    pair_j = torch.tensor([1, len(world), -1], dtype=torch.int32, device=dev)
    count = torch.zeros((3, 2), dtype=torch.int32, device=dev)
    sums = torch.zeros((3, 4), dtype=torch.float64, device=dev)
    assert lib.prh_link_stats(G.ptr(w), G.ptr(cum), len(world), 5, G.ptr(offsets), G.ptr(pair_j), 3, 1.0, G.ptr(count),
                              G.ptr(sums), dev.index, G.stream(dev)) == 0
    count, sums = count.cpu().numpy(), sums.cpu().numpy()
    assert (count[1:] == -1).all() and np.isnan(sums[1:]).all() and (count[0] >= 0).all() and np.isfinite(sums[0]).all()


# ------------------------------------------------------------------ reproducibility
def test_two_runs_are_bitwise_equal_and_far_pieces_change_nothing(golden_dir):
    g = _golden(golden_dir)
    world, frame = g["world_shifted"], g["piece_pose"]
    a = LK.link_pieces(world, frame, origin=ZERO)
    b = LK.link_pieces(world, frame, origin=ZERO)
    for k in a:
        assert a[k].tobytes() == b[k].tobytes(), k
    far = world[:30] + [0.0, 900.0, 0.0]
    c = LK.link_pieces(np.concatenate([world, far]), np.concatenate([frame, frame[:30]]), origin=ZERO)
    old = (c["pairs"] < 100).all(axis=1)
    assert old.sum() == len(a["edge"]) and not ((c["pairs"][:, 0] < 100) & (c["pairs"][:, 1] >= 100)).any()
    for k in a:
        assert c[k][old].tobytes() == a[k].tobytes(), k
    fa, na = LK.fuse_unmatched(g["pieces"], g["piece_pose"], g["poses"], return_nodes=True)
    fb, nb = LK.fuse_unmatched(g["pieces"], g["piece_pose"], g["poses"], return_nodes=True)
    for k in ("X", "W", "C", "spread", "world", "s", "d", "seg", "g", "offset", "cluster"):
        assert na[k].tobytes() == nb[k].tobytes(), k
    assert all(x.tobytes() == y.tobytes() for p, q in zip(fa, fb) for x, y in zip(p, q))


# ------------------------------------------------------------------ a detector run
LANE_Y = (-1.7, 1.9)


def _write_detector_drive(root):
    """4 poses 25 m apart with a little yaw, a ground cloud of 30 k points, and a results JSON whose
    pixels are two straight lanes as each frame's BEV sees them (ego |x| <= 24)."""
    from pointnet_refine_amd.pcd import write_pcd_host
    rng = np.random.default_rng(7)
    drive = root / "drive"
    (drive / "pose").mkdir(parents=True)
    n = 30000
    cloud = np.column_stack([rng.uniform(-8.0, 108.0, n), rng.uniform(-4.0, 4.0, n), rng.normal(0.0, 0.02, n),
                             rng.uniform(0.0, 60.0, n)])
    write_pcd_host(str(drive / "merged.pcd"), cloud)
    results = {}
    for k in range(4):
        ts = 1000 + k
        pose = np.array([25.0 * (k + 1), 0.3 * k, 0.0, *O.quat_yaw_pitch(0.04 * (k - 1.5), 0.0)])
        json.dump({"ts": str(ts), "x": pose[0], "y": pose[1], "z": pose[2], "qx": pose[3], "qy": pose[4], "qz": pose[5],
                   "qw": pose[6]}, open(drive / "pose" / f"{ts}.json", "w"))
        inst = []
        for y in LANE_Y:
            lane = np.stack([np.linspace(-10.0, 140.0, 601), np.full(601, y), np.zeros(601)], 1)
            ego = O.to_ego(lane, pose)
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


def test_refine_predictions_end_to_end(tmp_path):
    from pointnet_refine_amd.drive import load_gt_items
    drive = _write_detector_drive(tmp_path)
    res = LK.refine_predictions(_zero_head_model().cuda().eval(), str(drive), str(tmp_path / "results.json"))
    rep = res["report"]
    print(rep)
    assert rep["slices"] == 4 and rep["pieces"] == 8 and rep["pieces_sparse"] == 0 and rep["pieces_unlinked"] == 0
    assert rep["clusters"] == rep["clusters_kept"] == 2 and rep["edges"] >= 6 and rep["candidates"] >= rep["edges"]
    assert res["pieces"].shape == (8, 32, 3) and sorted(res["piece_frame"]) == [0, 0, 1, 1, 2, 2, 3, 3]
    assert res["pose_index"] == [0, 1, 2, 3] and res["poses"].shape == (4, 7)
    # the head is zero, so the map is the lanes: fp32 ulp at 100 m is 7.6e-6 and the path rounds a handful of times
    for parts in res["fused"]:
        assert len(parts) == 1 and len(parts[0]) > 200
        y = [abs(float(parts[0][:, 1].mean()) - v) for v in LANE_Y]
        assert min(y) <= 1e-4 and np.abs(parts[0][:, 1] - LANE_Y[int(np.argmin(y))]).max() <= 1e-4
    assert F.write_map_json(str(tmp_path / "direct.json"), res["fused"]) == 2
    assert len(load_gt_items(str(tmp_path / "direct.json"))) == 2


def test_example_runs_on_the_detector_drive(tmp_path):
    import subprocess
    import sys
    from pointnet_refine_amd.drive import load_gt_items
    drive = _write_detector_drive(tmp_path)
    ckpt = tmp_path / "model.pth"
    torch.save(_zero_head_model().state_dict(), ckpt)
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out = subprocess.run([sys.executable, os.path.join(root, "examples", "refine_predictions.py"), str(drive),
                          str(tmp_path / "results.json"), "--checkpoint", str(ckpt), "--out", str(tmp_path / "map.json"),
                          "--gt", str(tmp_path / "gt.json"), "--png", str(tmp_path / "png")], capture_output=True, text=True,
                         timeout=300)
    print(out.stdout[-2000:], out.stderr[-2000:])
    assert out.returncode == 0
    items = load_gt_items(str(tmp_path / "map.json"))
    assert len(items) == 2 and all(len(it["points"]) > 200 for it in items)
    assert sorted(it["attributes"]["source_line"] for it in items) == [0, 1]          # as many clusters as lanes
    assert "2 clusters" in out.stdout and "fused map" in out.stdout and os.path.getsize(tmp_path / "png" / "drive_map.png") > 1000
