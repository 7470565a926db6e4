"""Piece linking without a GPU: the restatement of the rule (_link_oracle.py) against what the rule
is for (one cluster per lane, whatever the direction and the order of the pieces, and a map closer
to the lanes than the pieces' noise), the host half of pointnet_refine_amd.link (step 6) against the
restatement, argument checks and the refusal to run without a device."""
import functools
import os

import numpy as np
import pytest
import torch

import _fuse_oracle as O
import _link_oracle as K
from pointnet_refine_amd import link as LK

BASE = np.array([400123.0, 3200456.0, 52.0])
IDENT = np.array([[0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 1.0]])
LINK_KEYS = ("pairs", "n_in", "n_out", "sum_d", "sum_self", "sum_other", "sum_dot", "edge", "rho", "delta")


@functools.lru_cache(maxsize=None)
def _golden():
    root = os.path.dirname(os.path.abspath(__file__))
    return dict(np.load(os.path.join(root, "golden", "g16_piece_links.npz")))


def _stored_links(g):
    return {k: g["link_" + k] for k in LINK_KEYS}


def _membership(cluster):
    """The clusters as a set of sets of piece numbers."""
    return {frozenset(np.flatnonzero(cluster == c).tolist()) for c in np.unique(cluster)}


@functools.lru_cache(maxsize=None)
def _world():
    g = _golden()
    ps = g["poses"].copy()
    ps[:, :3] -= g["origin"]
    return O.to_world(g["pieces"], g["piece_pose"], ps)


def test_fixture_is_the_case_the_maker_describes():
    g = _golden()
    pieces, piece_pose, poses, truth = K.make_case(int(g["seed"]), BASE)
    assert pieces.shape == (100, 32, 3) and len(poses) == 20
    for k, v in (("pieces", pieces), ("piece_pose", piece_pose), ("poses", poses), ("truth", truth)):
        assert np.array_equal(g[k], v), k
    assert np.array_equal(g["origin"], [400000.0, 3200000.0, 0.0])
    assert np.array_equal(_world(), g["world_shifted"]) and np.abs(g["world_shifted"]).max() < 2500.0
    assert 450 <= len(g["link_edge"]) <= 700 and 300 <= int(g["link_edge"].sum()) <= 450


def test_oracle_gives_one_pure_and_complete_cluster_per_lane():
    g = _golden()
    track = K.new_track()
    links = K.link(_world(), g["piece_pose"], track=track)
    marg = K.margins(track)
    print("margins:", marg)
    assert min(marg.values()) >= 1e-6
    for k in LINK_KEYS:
        assert np.array_equal(links[k], g["link_" + k]), k
    s = K.sync(100, links)
    assert np.array_equal(s["cluster"], g["clusters_all"])
    assert _membership(s["cluster"]) == _membership(g["truth"]) and len(_membership(s["cluster"])) == 4


def test_clusters_do_not_depend_on_piece_direction():
    g = _golden()
    links = K.link(_world()[:, ::-1], g["piece_pose"])
    assert _membership(K.sync(100, links)["cluster"]) == _membership(g["truth"])


def test_clusters_do_not_depend_on_piece_order():
    g = _golden()
    perm = np.random.default_rng(5).permutation(100)
    links = K.link(_world()[perm], g["piece_pose"][perm])
    cluster = K.sync(100, links)["cluster"]
    back = np.empty(100, dtype=np.int64)
    back[perm] = cluster                               # cluster of the original piece numbers
    assert _membership(back) == _membership(g["truth"])


def test_oracle_map_is_closer_to_the_lanes_than_the_noise():
    """A condition on the yardstick: the stored map (the oracle's steps 1-8) lies within the pieces'
    noise sigma of 0.05 m of the true lanes on average (measured 0.028-0.033 m over seeds 0-2)."""
    g = _golden()
    sizes = np.cumsum(g["fused_sizes"])[:-1]
    parts = np.split(g["fused_vertices"], sizes)
    assert sorted(g["fused_line"].tolist()) == [0, 1, 2, 3]            # one polyline per cluster
    for c, pts in zip(g["fused_line"], parts):
        lanes = np.unique(g["truth"][g["cluster"] == c])
        assert len(lanes) == 1
        d = K.distance_to_lane(pts, K.LANES[int(lanes[0])], BASE)
        print(f"cluster {c}: lane {lanes[0]}, {len(pts)} vertices, mean {d.mean():.4f} m, max {d.max():.4f} m")
        assert d.mean() < 0.05 and len(pts) > 400


def test_sync_pieces_is_the_oracles_step_six():
    g = _golden()
    links = _stored_links(g)
    got, want = LK.sync_pieces(100, links), K.sync(100, links)
    for k in ("cluster", "level", "parent", "sign"):
        assert np.array_equal(got[k], want[k]) and np.array_equal(got[k], g["clusters_all" if k == "cluster" else k]), k
    assert got["level"].max() >= 3 and (got["sign"] < 0).any() and (got["parent"] < 0).sum() == 4
    assert np.abs(got["offset"] - want["offset"]).max() <= 1e-9 and np.abs(got["offset"] - g["offset"]).max() <= 1e-9
    garc, flip = LK.arc_positions(g["cum"], got)
    assert np.abs(garc - K.arc(g["cum"], want)).max() <= 1e-9 and np.abs(garc - g["g"]).max() <= 1e-9
    assert np.array_equal(flip, want["sign"] < 0) and (np.diff(garc, axis=1) > 0).all() and garc.min() == 0.0


def test_sync_pieces_on_small_graphs():
    # no pieces, pieces without edges, and a tie in n_in that goes to the smaller parent
    empty = {"pairs": np.zeros((0, 2), dtype=np.int64), "edge": np.zeros(0, dtype=bool), "n_in": np.zeros(0, dtype=np.int32),
             "rho": np.zeros(0, dtype=np.int8), "delta": np.zeros(0)}
    assert all(len(v) == 0 for v in LK.sync_pieces(0, empty).values())
    lone = LK.sync_pieces(3, empty)
    assert lone["cluster"].tolist() == [0, 1, 2] and lone["parent"].tolist() == [-1, -1, -1]
    links = {"pairs": np.array([[0, 1], [0, 2], [1, 3], [2, 3], [3, 4], [5, 7], [6, 7]]),
             "edge": np.array([1, 1, 1, 1, 0, 1, 1], dtype=bool), "n_in": np.array([9, 8, 7, 7, 50, 5, 6], dtype=np.int32),
             "rho": np.array([1, -1, 1, -1, 1, -1, 1], dtype=np.int8),
             "delta": np.array([1.5, 20.0, 2.5, 30.0, 0.0, 4.0, 3.0])}
    got, want = LK.sync_pieces(8, links), K.sync(8, links)
    for k in got:
        assert np.array_equal(got[k], want[k]), k
    # 3 is reached from 1 and 2 with the same n_in: the smaller one is its parent; 6 hangs below 7, the j of its edge
    assert got["cluster"].tolist() == [0, 0, 0, 0, 1, 2, 2, 2] and got["parent"].tolist() == [-1, 0, 0, 1, -1, -1, 7, 5]
    assert got["level"].tolist() == [0, 1, 1, 2, 0, 0, 2, 1] and got["sign"].tolist() == [1, 1, -1, 1, 1, 1, -1, -1]
    assert got["offset"].tolist() == [0.0, 1.5, 20.0, 4.0, 0.0, 0.0, 7.0, 4.0]
    with pytest.raises(ValueError, match="outside"):
        LK.sync_pieces(3, links)


def test_host_step_five_matches_the_oracle():
    g = _golden()
    edge, rho, delta = LK.edges_of(g["link_n_in"], g["link_n_out"], g["link_sum_self"], g["link_sum_other"], g["link_sum_dot"])
    assert np.array_equal(edge, g["link_edge"]) and np.array_equal(rho, g["link_rho"])
    assert np.array_equal(delta, g["link_delta"]) and rho.dtype == np.int8
    assert np.array_equal(LK.piece_cums(g["world_shifted"]), g["cum"])


def test_argument_checks_come_before_the_device(monkeypatch):
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    with pytest.raises(ValueError, match=r"\(P,M,3\)"):
        LK.link_pieces(np.zeros((4, 3)), [0, 1, 2, 3])
    with pytest.raises(ValueError, match="points per piece"):
        LK.link_pieces(np.zeros((2, 1, 3)), [0, 1])
    with pytest.raises(ValueError, match="points per piece"):
        LK.link_pieces(np.zeros((2, 65, 3)), [0, 1])
    with pytest.raises(ValueError, match="piece_frame"):
        LK.link_pieces(np.zeros((2, 4, 3)), [0, 1, 2])
    with pytest.raises(ValueError, match="piece_frame"):
        LK.link_pieces(np.zeros((2, 4, 3)), [0.0, 1.0])
    with pytest.raises(ValueError, match="gate"):
        LK.link_pieces(np.zeros((2, 4, 3)), [0, 1], gate=-1.0)
    with pytest.raises(ValueError, match="points per piece"):
        LK.fuse_unmatched(np.zeros((2, 65, 3)), [0, 0], IDENT)
    with pytest.raises(ValueError, match="piece_pose"):
        LK.fuse_unmatched(np.zeros((2, 4, 3)), [0, 1], IDENT)
    with pytest.raises(ValueError, match="piece_pose"):
        LK.fuse_unmatched(np.zeros((2, 4, 3)), [0], IDENT)
    with pytest.raises(ValueError, match="step"):
        LK.fuse_unmatched(np.zeros((2, 4, 3)), [0, 0], IDENT, step=0.0)
    with pytest.raises(ValueError, match="quaternion"):
        LK.fuse_unmatched(np.zeros((2, 4, 3)), [0, 0], 2.0 * IDENT)


def test_device_functions_need_a_gpu(monkeypatch, tmp_path):
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    with pytest.raises(RuntimeError, match="needs a GPU"):
        LK.link_pieces(np.zeros((2, 4, 3)), [0, 1])
    with pytest.raises(RuntimeError, match="needs a GPU"):
        LK.fuse_unmatched(np.zeros((2, 4, 3)), [0, 0], IDENT)
    with pytest.raises(RuntimeError, match="needs a GPU"):
        LK.refine_predictions(None, str(tmp_path), str(tmp_path / "results.json"))


def test_library_exports_and_refuses_bad_arguments():
    from pointnet_refine_amd import _lib
    lib = _lib.lib()
    assert lib.prh_link_tile() >= 64 and lib.prh_link_tile() % 64 == 0 and 1 <= lib.prh_link_pairs_per_block() <= 16
    assert lib.prh_link_pairs_workspace_bytes(-1) == 0 and lib.prh_link_pairs_workspace_bytes(0) > 0
    assert lib.prh_link_pairs_count(None, 4, 1, None, 1.0, None, None, 0, 0, None) != 0       # M < 2
    assert lib.prh_link_pairs_count(None, 4, 65, None, 1.0, None, None, 0, 0, None) != 0
    assert lib.prh_link_stats(None, None, 4, 8, None, None, -1, 1.0, None, None, 0, None) != 0
    assert lib.prh_link_stats(None, None, 4, 8, None, None, 0, 1.0, None, None, 0, None) == 0  # no pairs: nothing to do
    assert lib.prh_link_stats(None, None, 4, 8, None, None, 5, 1.0, None, None, 0, None) != 0  # null pointers
