"""Steps 5-6 as the device runs them (_link_sync_oracle.py: min-label rounds with jumping, then per
tree level the maximum of a packed 64-bit key) against the host statement link.sync_pieces: all five
arrays equal, offset compared as bits.  No GPU: the links come from _link_oracle.link or are drawn."""
import numpy as np
import pytest

import _link_oracle as K
import _link_sync_oracle as S
from pointnet_refine_amd import link as LK

KEYS = ("cluster", "level", "parent", "sign", "offset")


def _assert_same(n_pieces, links, seeds=(0, 1)):
    want = LK.sync_pieces(n_pieces, links)
    for seed in seeds:                                 # the order the lowerings arrive in must not show
        got = S.sync(n_pieces, links, seed)
        for k in KEYS:
            assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape, k
            assert got[k].tobytes() == want[k].tobytes(), (k, seed)
    return got, want


def test_tie_goes_to_the_smaller_parent():
    world, frame = S.tie_case()
    links = K.link(world, frame)
    sel = np.flatnonzero(links["edge"])
    assert links["pairs"][sel].tolist() == [[0, 1], [0, 2], [1, 2], [1, 3], [2, 3], [3, 5]]
    assert links["n_in"][sel].tolist() == [8, 8, 18, 8, 8, 8]
    got, want = _assert_same(6, links)
    assert want["level"].tolist() == [0, 1, 1, 2, 0, 3]
    # the tie exists: D's two neighbours at level 1 offer the same n_in
    n_in = {tuple(p): int(n) for p, n in zip(links["pairs"][sel].tolist(), links["n_in"][sel])}
    assert want["level"][1] == want["level"][2] == 1 and n_in[(1, 3)] == n_in[(2, 3)]
    assert LK.parent_key(n_in[(1, 3)], 1) > LK.parent_key(n_in[(2, 3)], 2)
    assert got["parent"].tolist() == [-1, 0, 0, 1, -1, 3]
    assert got["cluster"].tolist() == [0, 0, 0, 0, 1, 0]               # the far piece is its own cluster 1
    assert got["sign"].tolist() == [1, 1, 1, 1, 1, -1] and got["level"][5] == 3


def test_chain_of_300_pieces():
    world, frame = S.chain_case(300, 5)
    links = K.link(world, frame)
    got, want = _assert_same(300, links, seeds=(0,))
    assert int(links["edge"].sum()) == 442 and want["cluster"].max() == 0 and want["level"].max() == 201
    assert got["levels"] == 201


@pytest.mark.parametrize("seed,n_groups,n_edges", [(1, 5, 260), (2, 7, 400), (3, 3, 400), (4, 11, 600)])
def test_random_edge_lists(seed, n_groups, n_edges):
    links = S.random_links(200, n_groups, n_edges, seed)
    got, want = _assert_same(200, links)
    assert want["cluster"].max() + 1 >= n_groups and (want["sign"] == -1).any() and want["level"].max() >= 3
    roots = np.flatnonzero(want["level"] == 0)
    assert (roots[:n_groups] == np.arange(n_groups)).all()             # the smallest members interleave
    # ties are everywhere: some child had two offers of its parent's n_in at the parent's level
    tied = 0
    nbr = {}
    for (i, j), n in zip(links["pairs"].tolist(), links["n_in"].tolist()):
        nbr.setdefault(i, []).append((j, n))
        nbr.setdefault(j, []).append((i, n))
    for b in range(200):
        if want["parent"][b] >= 0:
            offers = [(n, a) for a, n in nbr[b] if want["level"][a] == want["level"][b] - 1]
            best = max(n for n, _ in offers)
            tied += sum(1 for n, _ in offers if n == best) > 1
            assert want["parent"][b] == min(a for n, a in offers if n == best)
    assert tied >= 5


@pytest.mark.parametrize("n_pieces", [0, 1, 7])
def test_no_edges(n_pieces):
    links = {"pairs": np.zeros((0, 2), dtype=np.int64), "n_in": np.zeros(0, dtype=np.int32), "edge": np.zeros(0, dtype=bool),
             "rho": np.zeros(0, dtype=np.int8), "delta": np.zeros(0)}
    got, want = _assert_same(n_pieces, links)
    assert got["cluster"].tolist() == list(range(n_pieces)) and (got["level"] == 0).all() and got["rounds"] == 0
    # candidates that are no edges change nothing
    if n_pieces == 7:
        links = {"pairs": np.array([[0, 1], [2, 5]]), "n_in": np.array([3, 0], dtype=np.int32), "edge": np.zeros(2, dtype=bool),
                 "rho": np.ones(2, dtype=np.int8), "delta": np.array([1.0, 0.0])}
        _assert_same(7, links)


def test_parent_key_round_trip_and_order():
    for n_in, a in [(1, 0), (4, 17), (128, (1 << 24) - 1), (0, 0), ((1 << 31) - 1, 0xFFFFFFFF)]:
        k = LK.parent_key(n_in, a)
        assert 0 <= k < 1 << 64 and LK.parent_of_key(k) == (n_in, a)
    assert LK.parent_key(1, (1 << 24) - 1) > 0                          # 0 means no offer
    assert LK.parent_key(5, 900) > LK.parent_key(4, 0)                  # n_in first
    assert LK.parent_key(5, 3) > LK.parent_key(5, 4)                    # then the smaller index
    keys = sorted(((n, a) for n in (4, 5, 128) for a in (0, 1, 255, 256, 1 << 20)), key=lambda t: LK.parent_key(*t))
    assert keys == sorted(keys, key=lambda t: (t[0], -t[1]))
    for bad in [(-1, 0), (1 << 31, 0), (4, -1), (4, 1 << 32)]:
        with pytest.raises(ValueError):
            LK.parent_key(*bad)


def test_link_sync_checks_arguments_then_needs_a_gpu(monkeypatch):
    import torch
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    world, frame = S.tie_case()
    with pytest.raises(ValueError, match=r"\(P,M,3\)"):
        LK.link_sync(np.zeros((4, 3)), [0, 1, 2, 3])
    with pytest.raises(ValueError, match="min_in"):
        LK.link_sync(world, frame, min_in=0)
    with pytest.raises(RuntimeError, match="needs a GPU"):
        LK.link_sync(world, frame)
    ident = np.array([[0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 1.0]])
    with pytest.raises(RuntimeError, match="needs a GPU"):
        LK.fuse_unmatched(np.zeros((2, 4, 3)), [0, 0], ident, device_sync=True)


def test_library_refuses_bad_arguments():
    """Refusals that come before any device call, so they run without a GPU."""
    from pointnet_refine_amd import _lib
    lib = _lib.lib()
    assert lib.prh_link_edges_blocks(-1) == 0 and lib.prh_link_edges_blocks(0) == 0 and lib.prh_link_edges_blocks(1) == 1
    assert lib.prh_link_edges_blocks(257) == lib.prh_link_edges_blocks(256) + 1
    assert lib.prh_link_cum(None, 4, 1, None, 0, None) != 0                    # M < 2
    assert lib.prh_link_cum(None, 4, 65, None, 0, None) != 0
    assert lib.prh_link_cum(None, 0, 8, None, 0, None) == 0                    # no pieces: nothing to do
    assert lib.prh_link_cum(None, 4, 8, None, 0, None) != 0                    # null pointers
    assert lib.prh_link_edges(None, 4, None, None, 5, 0, 4, None, None, None, None, None, 0, None) != 0     # min_in < 1
    assert lib.prh_link_edges(None, 4, None, None, 5, 4, -1, None, None, None, None, None, 0, None) != 0
    assert lib.prh_link_edges(None, 4, None, None, 5, 4, 4, None, None, None, None, None, 0, None) != 0     # null
    assert lib.prh_link_edges_compact(None, None, None, None, None, None, 4, None, 5, None, None, None, 0, None) != 0
    assert lib.prh_link_edges_compact(None, None, None, None, None, None, 4, None, 0, None, None, None, 0, None) == 0
    assert lib.prh_link_label_round(None, 3, (1 << 24) + 1, None, None, 0, None) != 0
    assert lib.prh_link_label_round(None, 3, 4, None, None, 0, None) != 0      # null pointers
    assert lib.prh_link_tree_init(None, 0, None, None, None, None, None, 0, None) == 0
    assert lib.prh_link_tree_init(None, 4, None, None, None, None, None, 0, None) != 0
    assert lib.prh_link_tree_level(None, None, None, 3, 4, -1, None, None, None, None, None, None, 0, None) != 0
    assert lib.prh_link_tree_level(None, None, None, 3, 4, 0, None, None, None, None, None, None, 0, None) != 0
