"""Map fusion without a GPU: the numpy restatement of the rule (_fuse_oracle.py) against the
properties the rule promises, the host half of pointnet_refine_amd.fuse (step 6, the map file, the
origin, argument checks) and the refusal to run without a device."""
import math
import os

import numpy as np
import pytest
import torch

import _fuse_oracle as O
from pointnet_refine_amd import fuse as F
from pointnet_refine_amd.drive import load_gt_items

IDENT = np.array([[0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 1.0]])


def _straight(n=21, length=100.0):
    return np.stack([np.linspace(0.0, length, n), np.full(n, 2.0), np.zeros(n)], 1)


def _golden(golden_dir):
    g = np.load(os.path.join(golden_dir, "g15_map_fusion.npz"))
    off = g["line_offsets"]
    return g, [g["line_vertices"][off[l]:off[l + 1]] for l in range(len(off) - 1)]


def test_fixture_is_what_the_oracle_gives(golden_dir):
    g, lines = _golden(golden_dir)
    assert os.path.getsize(os.path.join(golden_dir, "g15_map_fusion.npz")) < 200 * 1024
    assert len(g["poses"]) == 3 and len(lines) == 4 and 35 <= len(g["pieces"]) <= 45
    r = O.fuse(lines, g["pieces"], g["piece_line"], g["piece_pose"], g["poses"], float(g["step"]))
    assert np.array_equal(r["origin"], g["origin"]) and np.array_equal(r["origin"], [400000.0, 3200000.0, 0.0])
    assert np.array_equal(r["C"], g["C"]) and np.array_equal(r["seg"], g["seg"])
    for k in ("world", "s", "d", "X", "W", "spread"):
        assert np.abs(r[k] - g[k]).max() <= 1e-9, k
    # the conditions the maker asserted, restated on the stored arrays
    shifted = [l - g["origin"] for l in lines]
    cums = [O.carrier_cum(v) for v in shifted]
    node_m, seg_m = O.margins(shifted, cums, g["world"] - g["origin"], g["piece_line"], g["s"], float(g["step"]))
    assert node_m >= 1e-6 and seg_m >= 1e-6
    # one piece runs against its carrier (no contribution), one doubles back
    ds = np.diff(g["s"], axis=1)
    assert ((ds <= 0).all(axis=1)).sum() == 1 and (((ds < 0).any(axis=1)) & ((ds > 0).any(axis=1))).sum() >= 1


def test_carrier_cum_has_the_oracles_bits():
    rng = np.random.default_rng(3)
    v = O.curved_carrier(300, [123.0, -45.0, 6.0], rng)
    assert np.array_equal(F.carrier_cum(v), O.carrier_cum(v))
    assert F.carrier_cum(np.zeros((0, 3))).shape == (0,) and np.array_equal(F.carrier_cum(np.ones((1, 3))), [0.0])


def test_straight_carrier_is_reproduced():
    line = _straight()
    rng = np.random.default_rng(0)
    poses = O.make_poses(3, [20.0, 0.0, 0.0], rng)
    pieces = np.stack([O.make_piece(line, poses[k], np.linspace(3.3 + 25 * k, 44.1 + 25 * k, 32), rng, 0.0) for k in range(3)])
    r = O.fuse([line], pieces, [0, 0, 0], [0, 1, 2], poses, origin=np.zeros(3))
    used = np.flatnonzero(r["C"] > 0)
    assert len(used) > 150 and r["C"].max() == 2
    want = np.stack([used * 0.5, np.full(len(used), 2.0), np.zeros(len(used))], 1)
    assert np.abs(r["X"][used] - want).max() <= 1e-9
    assert r["d"].max() <= 1e-9 and r["spread"].max() <= 1e-9
    assert len(r["fused"][0]) == 1 and len(r["fused"][0][0]) == len(used)


def test_curved_carrier_within_its_chord_bound():
    # a circle of radius R sampled every h metres: a chord's midpoint lies h^2 / (8 R) inside the
    # arc, and the piece's own 1.3 m chords add as much again
    R, n = 200.0, 400
    ang = np.linspace(0.0, 100.0 / R, n)
    line = np.stack([R * np.sin(ang), R * (1 - np.cos(ang)), np.zeros(n)], 1)
    pieces = np.stack([O.make_piece(line, IDENT[0], np.linspace(2.2 + 25 * k, 42.7 + 25 * k, 32), None, 0.0) for k in range(3)])
    r = O.fuse([line], pieces, [0, 0, 0], [0, 0, 0], IDENT, origin=np.zeros(3))
    used = np.flatnonzero(r["C"] > 0)
    bound = (40.5 / 31) ** 2 / (8 * R) + (100.0 / (n - 1)) ** 2 / (8 * R) + 1e-9
    radial = np.abs(np.hypot(r["X"][used, 0], r["X"][used, 1] - R) - R)
    assert len(used) > 150 and radial.max() <= bound and np.abs(r["X"][used, 2]).max() <= 1e-12


def test_reversed_piece_contributes_nothing_and_backtrack_twice():
    line = _straight()
    rng = np.random.default_rng(1)
    fwd = O.make_piece(line, IDENT[0], np.linspace(10.2, 30.1, 32), rng, 0.02)
    both = O.fuse([line], np.stack([fwd, fwd[::-1]]), [0, 0], [0, 0], IDENT, origin=np.zeros(3))
    one = O.fuse([line], fwd[None], [0], [0], IDENT, origin=np.zeros(3))
    for k in ("X", "W", "C", "spread"):
        assert np.array_equal(both[k], one[k]), k
    assert one["C"].max() >= 1
    back = O.make_piece(line, IDENT[0], np.concatenate([np.linspace(10.2, 30.1, 20), np.linspace(29.3, 20.4, 6),
                                                        np.linspace(21.2, 35.3, 6)]), rng, 0.0)
    r = O.fuse([line], back[None], [0], [0], IDENT, origin=np.zeros(3))
    assert r["C"][int(25 / 0.5)] == 2 and r["C"][int(15 / 0.5)] == 1 and r["C"][int(33 / 0.5)] == 1


def test_taper_and_weights():
    assert [O.taper(i, 5) for i in range(5)] == [1.0, 2.0, 3.0, 2.0, 1.0]
    assert [O.taper(i, 4) for i in range(4)] == [1.0, 2.0, 2.0, 1.0]
    assert [O.taper(i, 2) for i in range(2)] == [1.0, 1.0]
    # one piece of 5 points at s = 1, 3, 5, 7, 9 on a straight line: W at a node is the taper
    # interpolated along the piece segment the node falls in
    line = _straight(3, 10.0)
    piece = np.stack([np.array([1.0, 3.0, 5.0, 7.0, 9.0]), np.full(5, 2.0), np.zeros(5)], 1)
    r = O.fuse([line], piece[None], [0], [0], IDENT, step=0.5, origin=np.zeros(3))
    assert r["W"][2] == 1.0 and r["W"][4] == 1.5 and r["W"][10] == 3.0 and r["W"][13] == 2.25
    assert r["C"][1] == 0 and r["C"][18] == 0 and r["C"][17] == 1       # s[i] <= j ds < s[i+1]: 9.0 is outside


def test_polylines_split_and_min_count():
    C = np.array([0, 1, 1, 1, 0, 0, 0, 2, 2, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 1, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 3, 3])
    X = np.arange(len(C) * 3, dtype=np.float64).reshape(-1, 3)
    for fn in (O.polylines, F.node_polylines):
        # 3 -> 7 is 2 m (kept together), 8 -> 19 is 5.5 m (split), the single node 19 is dropped
        runs = fn(X, C, 0.5, 1, 5.0)
        assert [len(r) for r in runs] == [5, 2]
        assert np.array_equal(runs[0], X[[1, 2, 3, 7, 8]]) and np.array_equal(runs[1], X[[31, 32]])
        assert [len(r) for r in fn(X, C, 0.5, 2, 5.0)] == [2, 2]
        assert [len(r) for r in fn(X, C, 0.5, 1, 1.0)] == [3, 2, 2]
        assert [len(r) for r in fn(X, C, 0.5, 1, 100.0)] == [8]
        assert fn(X, np.zeros_like(C), 0.5, 1, 5.0) == []
    # exactly max_gap apart stays together
    assert [len(r) for r in F.node_polylines(X, np.array([1] + [0] * 9 + [1]), 0.5, 1, 5.0)] == [2]


def test_write_map_json_round_trip(tmp_path):
    rng = np.random.default_rng(2)
    fused = [[rng.normal(size=(5, 3)) + [4e5, 3.2e6, 50.0], rng.normal(size=(2, 3))], [], [rng.normal(size=(7, 3))]]
    path = str(tmp_path / "map.json")
    n = F.write_map_json(path, fused, categories=["lane", "kerb", "lane"], attributes=[{"colour": "white"}, {}, {}])
    items = load_gt_items(path)
    assert n == 3 and len(items) == 3
    flat = [(l, k, p) for l, parts in enumerate(fused) for k, p in enumerate(parts)]
    for it, (l, k, p) in zip(items, flat):
        assert np.array_equal(it["points"], p)                         # repr round trip of doubles is exact
        assert it["attributes"]["source_line"] == l and it["attributes"]["part"] == k
    assert items[0]["category"] == "lane" and items[0]["attributes"]["colour"] == "white" and items[2]["category"] == "lane"
    F.write_map_json(path, [[], []])
    assert load_gt_items(path) == []


def test_origin_is_subtracted_and_added_back():
    assert np.array_equal(F.default_origin([[400123.4, 3200456.7, 52.0, 0, 0, 0, 1]]), [400000.0, 3200000.0, 0.0])
    assert np.array_equal(F.default_origin([[-0.5, 999.9, -1000.0, 0, 0, 0, 1]]), [-1000.0, 0.0, -1000.0])
    assert np.array_equal(F.default_origin(np.zeros((0, 7))), np.zeros(3))
    assert np.array_equal(O.default_origin([[400123.4, 3200456.7, 52.0, 0, 0, 0, 1]]), [400000.0, 3200000.0, 0.0])
    # the oracle far from zero, with its default origin, against the same drive moved to zero
    rng = np.random.default_rng(4)
    far = np.array([400000.0, 3200000.0, 0.0])
    poses = O.make_poses(2, [30.0, 0.0, 0.0], rng)
    line = O.curved_carrier(50, [0.0, 0.0, 0.0], rng)
    pieces = np.stack([O.make_piece(line, poses[k], np.linspace(4.1 + 25 * k, 47.3 + 25 * k, 16), rng, 0.03) for k in range(2)])
    near = O.fuse([line], pieces, [0, 0], [0, 1], poses, origin=np.zeros(3))
    poses_far = poses.copy()
    poses_far[:, :3] += far
    moved = O.fuse([line + far], pieces, [0, 0], [0, 1], poses_far)
    assert np.array_equal(moved["origin"], far) and np.array_equal(moved["C"], near["C"])
    assert np.abs(moved["X_shifted"] - near["X_shifted"]).max() <= 1e-9       # exact shifts: integers below 2^53
    used = near["C"] > 0
    assert np.abs(moved["X"][used] - far - near["X"][used]).max() <= 1e-9 and np.all(moved["X"][~used] == 0.0)


def test_argument_checks_come_before_the_device():
    line = _straight()
    ok = np.zeros((2, 4, 3))
    with pytest.raises(ValueError, match="points per piece"):
        F.fuse_pieces([line], np.zeros((2, 1, 3)), [0, 0], [0, 0], IDENT)
    with pytest.raises(ValueError, match="points per piece"):
        F.fuse_pieces([line], np.zeros((2, 65, 3)), [0, 0], [0, 0], IDENT)
    with pytest.raises(ValueError, match=r"\(P,M,3\)"):
        F.fuse_pieces([line], np.zeros((2, 4, 2)), [0, 0], [0, 0], IDENT)
    with pytest.raises(ValueError, match="piece_line"):
        F.fuse_pieces([line], ok, [0, 1], [0, 0], IDENT)
    with pytest.raises(ValueError, match="piece_line"):
        F.fuse_pieces([line], ok, [0], [0, 0], IDENT)
    with pytest.raises(ValueError, match="piece_line"):
        F.fuse_pieces([line], ok, [0.0, 0.5], [0, 0], IDENT)
    with pytest.raises(ValueError, match="piece_pose"):
        F.fuse_pieces([line], ok, [0, 0], [0, -1], IDENT)
    with pytest.raises(ValueError, match="piece_pose"):
        F.fuse_pieces([line], ok, [0, 0], [0, 1], IDENT)
    with pytest.raises(ValueError, match="quaternion of norm"):
        F.fuse_pieces([line], ok, [0, 0], [0, 0], [[0, 0, 0, 0, 0, 0, 1.001]])
    with pytest.raises(ValueError, match="quaternion of norm"):
        F.pieces_to_world(ok, [0, 0], [[0, 0, 0, 0, 0, 0, 0.0]])
    with pytest.raises(ValueError, match="step"):
        F.fuse_pieces([line], ok, [0, 0], [0, 0], IDENT, step=0.0)
    with pytest.raises(ValueError, match="no vertex"):
        F.fuse_pieces([np.zeros((0, 3))], ok, [0, 0], [0, 0], IDENT)
    with pytest.raises(ValueError, match="point_line"):
        F.project_to_lines(np.zeros((3, 3)), [0, 0, 2], [line, line])
    with pytest.raises(ValueError, match=r"\(N,3\)"):
        F.project_to_lines(np.zeros((3, 2)), [0, 0, 0], [line])
    with pytest.raises(ValueError, match="one list of polylines per line"):
        F.map_error([[]], [line, line])


def test_limits_match_the_library():
    from pointnet_refine_amd import _lib
    _lib.build()
    lib = _lib.lib()
    assert lib.prh_fuse_max_points() == F.MAX_POINTS == 64
    assert lib.prh_fuse_tile() >= 64
    assert lib.prh_fuse_project_workspace_bytes(0) > 0
    assert lib.prh_fuse_project_workspace_bytes(100) >= 100 * (12 * 8 + 2 * 4)     # a pose: t[3], m[9] fp64, fx, fy fp32
    assert lib.prh_fuse_gather_workspace_bytes(1000) >= 1000 * 16
    assert lib.prh_fuse_project_workspace_bytes(-1) == 0 and lib.prh_fuse_gather_workspace_bytes(-1) == 0


def test_device_functions_need_a_gpu(monkeypatch):
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    line = _straight()
    with pytest.raises(RuntimeError, match="needs a GPU"):
        F.fuse_pieces([line], np.zeros((1, 4, 3)), [0], [0], IDENT)
    with pytest.raises(RuntimeError, match="needs a GPU"):
        F.pieces_to_world(np.zeros((1, 4, 3)), [0], IDENT)
    with pytest.raises(RuntimeError, match="needs a GPU"):
        F.project_to_lines(np.zeros((2, 3)), [0, 0], [line])
    with pytest.raises(RuntimeError, match="needs a GPU"):
        F.map_error([[line]], [line])
    with pytest.raises(RuntimeError, match="needs a GPU"):
        F.refine_drive(None, np.zeros((4, 4), dtype=np.float32), np.zeros((2, 7)), [line])
