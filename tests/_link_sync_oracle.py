"""The device algorithm of steps 5-6 (csrc/prh_link_sync.hpp) in plain Python ints, and the cases
the CPU and the GPU tests share.  Components: rounds of "every edge lowers either end's label to
the other's" (in place, the edges in a shuffled order, as atomics arrive in any order) followed by
chasing every label to a label that is its own, until a round lowers nothing.  Trees: per level the
maximum of the packed key link.parent_key(n_in, a) over the neighbours a at that level, then the
edge whose key won places the child.  The rule itself is restated in _link_oracle.py."""
import random

import numpy as np

import _link_oracle as K
from pointnet_refine_amd import link as LK


def edge_list(links):
    """[(i, j, n_in, rho, delta)] of the candidates with 'edge', in candidate order."""
    sel = np.flatnonzero(np.asarray(links["edge"], dtype=bool))
    return [(int(links["pairs"][e][0]), int(links["pairs"][e][1]), int(links["n_in"][e]), int(links["rho"][e]),
             float(links["delta"][e])) for e in sel]


def components(n_pieces, edges, seed=0):
    """(label per piece, rounds run): the smallest member of every piece's component."""
    rng = random.Random(seed)
    label = list(range(n_pieces))
    rounds = 0
    while edges:
        rounds += 1
        lowered = False
        order = list(range(len(edges)))
        rng.shuffle(order)
        for e in order:
            i, j = edges[e][0], edges[e][1]
            li, lj = label[i], label[j]
            if lj < li:
                label[i], lowered = lj, True
            elif li < lj:
                label[j], lowered = li, True
        for p in range(n_pieces):
            l = label[p]
            while label[l] != l:
                l = label[l]
            label[p] = l
        if not lowered:
            break
        assert rounds <= n_pieces + 1
    return label, rounds


def sync(n_pieces, links, seed=0):
    """link.sync_pieces' dict plus 'levels' and 'rounds', by the device algorithm."""
    edges = edge_list(links)
    label, rounds = components(n_pieces, edges, seed)
    roots = [p for p in range(n_pieces) if label[p] == p]
    rank = {r: k for k, r in enumerate(roots)}
    level = [0 if label[p] == p else -1 for p in range(n_pieces)]
    parent, sign, offset, key = [-1] * n_pieces, [1] * n_pieces, [0.0] * n_pieces, [0] * n_pieces
    n = 0
    while edges and n < n_pieces:
        for i, j, n_in, _, _ in edges:                 # propose
            if level[i] == n and level[j] < 0:
                key[j] = max(key[j], LK.parent_key(n_in, i))
            elif level[j] == n and level[i] < 0:
                key[i] = max(key[i], LK.parent_key(n_in, j))
        placed = []
        for i, j, n_in, rho, delta in edges:           # place
            if level[i] == n and level[j] != n and key[j] == LK.parent_key(n_in, i):
                a, b = i, j
            elif level[j] == n and level[i] != n and key[i] == LK.parent_key(n_in, j):
                a, b = j, i
            else:
                continue
            assert level[b] < 0 and b not in placed    # one writer per child
            placed.append(b)
            parent[b], sign[b] = a, rho * sign[a]
            offset[b] = offset[a] + sign[a] * delta if a == i else offset[a] - sign[b] * delta
        for b in placed:
            level[b] = n + 1
        if not placed:
            break
        n += 1
    return {"cluster": np.array([rank[l] for l in label], dtype=np.int64), "level": np.array(level, dtype=np.int64),
            "parent": np.array(parent, dtype=np.int64), "sign": np.array(sign, dtype=np.int8),
            "offset": np.array(offset, dtype=np.float64), "levels": n, "rounds": rounds}


# ------------------------------------------------------------------ cases
def straight(x0, y, reverse=False, m=11, length=10.0):
    x = np.linspace(x0, x0 + length, m)
    p = np.stack([x, np.full(m, y), np.zeros(m)], 1)
    return p[::-1].copy() if reverse else p


def tie_case():
    """Six straight pieces of 11 points over 10 m: A at x = 0, B and its copy C at x = 6, y = 0.1, D at
    x = 12, a far piece at x = 100 and a reversed piece at x = 18, y = 0.05; frames 0..5.  D has two
    level-1 neighbours of equal n_in."""
    world = np.stack([straight(0.0, 0.0), straight(6.0, 0.1), straight(6.0, 0.1), straight(12.0, 0.0),
                      straight(100.0, 0.0), straight(18.0, 0.05, reverse=True)])
    return world, np.arange(6)


def chain_case(n_pieces, seed):
    """tests/test_link_gpu.py::_chain_case restated: short pieces of 3 points along one line, 0.7 m
    apart, 7 frames in turn."""
    rng = np.random.default_rng(seed)
    world = np.zeros((n_pieces, 3, 3))
    for p in range(n_pieces):
        x = 0.7 * p + np.array([0.0, 1.4, 3.1])
        world[p] = np.stack([x, 0.05 * np.sin(x) + 5.0, np.zeros(3)], 1) + rng.normal(0.0, 0.02, (3, 3))
    return world, np.arange(n_pieces) % 7


def crossing_case():
    """test_link_gpu's 130 two-point pieces across one another in a 6 m patch, 5 frames, restated."""
    rng = np.random.default_rng(77)
    a = rng.uniform(0.0, 6.28, 130)
    centre = rng.uniform(-1.0, 1.0, (130, 2))
    d = np.stack([np.cos(a), np.sin(a)], 1) * rng.uniform(2.0, 3.0, (130, 1))
    world = np.zeros((130, 2, 3))
    world[:, 0, :2], world[:, 1, :2] = centre - d, centre + d
    return world, np.arange(130) % 5


def lanes_case(m, seed):
    """test_link_gpu's _lanes_case restated: three lanes from 6 frames, 18 pieces of m points."""
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


def random_links(n_pieces, n_groups, n_edges, seed):
    """A random edge list as a links dict: pieces p with p % n_groups equal form a group (so the
    groups' smallest members interleave), edges only inside a group, n_in from {4, 5} so ties are
    everywhere, rho and delta random.  Pairs are unique, i < j, in the candidates' order."""
    rng = np.random.default_rng(seed)
    pairs = set()
    while len(pairs) < n_edges:
        i, j = (int(v) for v in rng.integers(0, n_pieces, 2))
        if i != j and i % n_groups == j % n_groups:
            pairs.add((min(i, j), max(i, j)))
    pairs = np.array(sorted(pairs), dtype=np.int64)
    n = len(pairs)
    return {"pairs": pairs, "n_in": rng.integers(4, 6, n).astype(np.int32), "edge": np.ones(n, dtype=bool),
            "rho": rng.choice(np.array([-1, 1], dtype=np.int8), n), "delta": rng.normal(0.0, 5.0, n)}
