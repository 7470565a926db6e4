"""Steps 5-6 and cum on the GPU (csrc/prh_link_sync.hpp through link.link_sync) against the host
statement of the same rule: link.link_pieces + link.piece_cums + link.sync_pieces on the same input.
Both sides round every operation once in the same order, so nothing here has a tolerance: integer
arrays are compared for equality and every float array (cum, the sums, delta, offset, g, the map)
as bits."""
import functools
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import _fuse_oracle as O
import _link_oracle as K
import _link_sync_oracle as S
from pointnet_refine_amd import fuse as F
from pointnet_refine_amd import link as LK

pytestmark = pytest.mark.gpu
ZERO = np.zeros(3)
BASE = np.array([400123.0, 3200456.0, 52.0])
SYNC_KEYS = ("cluster", "level", "parent", "sign", "offset")
LINK_KEYS = ("pairs", "n_in", "n_out", "sum_d", "sum_self", "sum_other", "sum_dot", "edge", "rho", "delta")


def _same(a, b, what):
    a, b = np.asarray(a), np.asarray(b)
    assert a.dtype == b.dtype and a.shape == b.shape, (what, a.dtype, b.dtype, a.shape, b.shape)
    assert a.tobytes() == b.tobytes(), what


def _check(world, frame, origin=ZERO, **kw):
    """link_sync(return_links=True) against link_pieces + sync_pieces + piece_cums.  Returns (got, links)."""
    world = np.asarray(world, dtype=np.float64)
    links = LK.link_pieces(world, frame, origin=origin, **kw)
    want = LK.sync_pieces(len(world), links)
    got = LK.link_sync(world, frame, origin=origin, return_links=True, **kw)
    print("pieces:", len(world), "candidates:", got["candidates"], "edges:", got["edges"],
          "levels:", int(want["level"].max(initial=0)))
    for k in LINK_KEYS:
        _same(got["links"][k], links[k], "links." + k)
    for k in SYNC_KEYS:
        _same(got[k], want[k], k)
    shift = origin if origin is not None else np.floor(world[0, 0] / 1000.0) * 1000.0      # link_pieces' default
    _same(got["cum"], LK.piece_cums(world - shift), "cum")
    assert got["candidates"] == len(links["edge"]) and got["edges"] == int(links["edge"].sum())
    assert "links" not in LK.link_sync(world, frame, origin=origin, **kw)
    return got, links


@functools.lru_cache(maxsize=None)
def _golden():
    root = os.path.dirname(os.path.abspath(__file__))
    return dict(np.load(os.path.join(root, "golden", "g16_piece_links.npz")))


# ------------------------------------------------------------------ against the host statement
def test_fixture():
    g = _golden()
    got, _ = _check(g["world_shifted"], g["piece_pose"])
    assert got["cluster"].max() == 3 and got["edges"] >= 300
    for k in ("level", "parent", "sign"):
        assert np.array_equal(got[k], g[k]), k
    # from the drive frame proper, 400 km from zero, with the default origin (the subtraction rounds,
    # so the bits are compared with the host's on that input, not with the shifted run's)
    far, _ = _check(g["world_shifted"] + g["origin"], g["piece_pose"], origin=None)
    for k in ("cluster", "level", "parent", "sign"):
        _same(far[k], got[k], k)


def test_tie_goes_to_the_smaller_parent():
    world, frame = S.tie_case()
    got, links = _check(world, frame)
    sel = np.flatnonzero(links["edge"])
    assert links["pairs"][sel].tolist() == [[0, 1], [0, 2], [1, 2], [1, 3], [2, 3], [3, 5]]
    assert links["n_in"][sel].tolist() == [8, 8, 18, 8, 8, 8]          # the tie: (1,3) and (2,3) offer D the same
    assert got["level"].tolist() == [0, 1, 1, 2, 0, 3] and got["parent"].tolist() == [-1, 0, 0, 1, -1, 3]
    assert got["cluster"].tolist() == [0, 0, 0, 0, 1, 0] and got["sign"].tolist() == [1, 1, 1, 1, 1, -1]


def test_chain_of_300_pieces():
    world, frame = S.chain_case(300, 5)
    got, _ = _check(world, frame)
    assert got["edges"] == 442 and got["cluster"].max() == 0 and got["level"].max() == 201   # a launch pair per level


def test_rows_longer_than_a_ballot_word():
    world, frame = S.crossing_case()
    got, links = _check(world, frame)
    assert np.bincount(links["pairs"][:, 0]).max() > 64 and got["candidates"] > 6000
    _check(world, frame, min_in=1, out_ratio=0)                          # every candidate that touches is an edge
    _check(world, frame, min_in=2, out_ratio=1)


@pytest.mark.parametrize("m", [2, 5, 32, 33, 64])
def test_points_per_piece(m):
    world, frame = S.lanes_case(m, 200 + m)
    got, _ = _check(world, frame)
    if m > 2:
        assert got["cluster"].max() == 2 and got["edges"] >= 20 and (got["sign"] == -1).any()


@pytest.mark.parametrize("n_pieces", [0, 1, 2, 257])
def test_piece_counts(n_pieces):
    """No piece, no pair, one pair, and one piece past a block of the per-piece kernels."""
    world, frame = S.chain_case(n_pieces, 300 + n_pieces)
    got, _ = _check(world, frame)
    assert got["cum"].shape == (n_pieces, 3) and got["offset"].shape == (n_pieces,)
    if n_pieces < 2:
        assert got["candidates"] == 0 and got["edges"] == 0 and got["cluster"].tolist() == list(range(n_pieces))
    if n_pieces == 257:
        assert got["candidates"] % 256 != 0 and got["cluster"].max() == 0


# ------------------------------------------------------------------ degenerate and edge inputs
def test_repeated_points_and_loose_parameters():
    base = S.straight(0.0, 0.0, m=6)
    dup = S.straight(1.0, 0.3, m=6)
    dup[3] = dup[2]                                    # a zero-length segment inside
    point = np.repeat(S.straight(5.1, 1.4, m=6)[:1], 6, axis=0)         # no usable segment at all: cum is all zero
    anti = S.straight(2.0, 0.2, reverse=True, m=6)
    world = np.stack([base, dup, point, anti])
    frame = np.arange(4)
    got, _ = _check(world, frame)
    assert (got["cum"][2] == 0.0).all() and got["cum"][1][3] == got["cum"][1][2]
    assert got["cluster"].tolist() == [0, 0, 1, 0] and got["sign"][3] == -1
    got, links = _check(world, frame, min_in=1, out_ratio=0)
    assert got["edges"] == int((links["n_in"] >= 1).sum())


def _edges_direct(offsets, count, sums, n_pieces, min_in=4, out_ratio=4):
    from pointnet_refine_amd import _gpu as G
    dev = torch.device("cuda", torch.cuda.current_device())
    off_t = torch.tensor(offsets, dtype=torch.int64, device=dev)
    cnt_t = torch.tensor(count, dtype=torch.int32, device=dev).reshape(-1, 2)
    sum_t = torch.tensor(sums, dtype=torch.float64, device=dev).reshape(-1, 4)
    pair_j = torch.zeros((cnt_t.shape[0],), dtype=torch.int32, device=dev)
    per, edges = LK.device_edges(dev, n_pieces, off_t, pair_j, cnt_t, sum_t, min_in, out_ratio)
    return {k: v.cpu().numpy() for k, v in per.items()}, {k: v.cpu().numpy() for k, v in edges.items()}


def test_sign_of_zero_and_nan_at_the_entry_point():
    nan = float("nan")
    count = [[8, 0], [8, 0], [8, 0], [8, 0], [0, 3], [-1, -1], [8, 3]]
    sums = [[1.0, 10.0, 4.0, 0.0], [1.0, 10.0, 4.0, -0.0], [1.0, 10.0, 4.0, nan], [1.0, 10.0, 4.0, -1e-300],
            [0.0, 0.0, 0.0, 0.0], [nan, nan, nan, nan], [1.0, 3.0, 1.0, 2.0]]
    per, edges = _edges_direct([0, 3, 3, 6, 7], count, sums, 4)
    want = LK.edges_of(np.array(count)[:, 0], np.array(count)[:, 1], np.array(sums)[:, 1], np.array(sums)[:, 2],
                       np.array(sums)[:, 3])
    assert per["rho"].tolist() == [1, 1, -1, -1, 1, -1, 1] == want[1].tolist()
    assert per["edge"].tolist() == [1, 1, 1, 1, 0, 0, 0] == want[0].astype(int).tolist()
    _same(per["delta"], want[2], "delta")
    assert per["delta"].tolist() == [0.75, 0.75, 1.75, 1.75, 0.0, 0.0, 0.25]
    assert per["pair_i"].tolist() == [0, 0, 0, 2, 2, 2, 3]             # the owner skips the empty row 1
    assert edges["ij"][:, 0].tolist() == [0, 0, 0, 2] and edges["w"].tolist() == [[8, 1], [8, 1], [8, -1], [8, -1]]
    _same(edges["delta"], want[2][:4], "edge delta")


def test_pair_outside_the_pieces_is_no_edge():
    """prh_link_stats gives counts of -1 for a pair_j that names no piece; step 5 must not make it an
    edge even with min_in = 1 and out_ratio = 0, and the compacted list must not hold it."""
    from pointnet_refine_amd import _gpu as G
    from pointnet_refine_amd import _lib
    lib = _lib.lib()
    world, _ = S.lanes_case(5, 205)
    n_p = len(world)
    dev = torch.device("cuda", torch.cuda.current_device())
    w = torch.from_numpy(world).to(dev)
    cum = LK.device_cums(dev, w)
    _same(cum.cpu().numpy(), LK.piece_cums(world), "cum")
    offsets = torch.tensor([0, 3] + [3] * (n_p - 1), dtype=torch.int64, device=dev)
    pair_j = torch.tensor([1, n_p, -1], dtype=torch.int32, device=dev)
    count = torch.zeros((3, 2), dtype=torch.int32, device=dev)
    sums = torch.zeros((3, 4), dtype=torch.float64, device=dev)
    assert lib.prh_link_stats(G.ptr(w), G.ptr(cum), n_p, 5, G.ptr(offsets), G.ptr(pair_j), 3, 1.0, G.ptr(count),
                              G.ptr(sums), dev.index, G.stream(dev)) == 0
    per, edges = LK.device_edges(dev, n_p, offsets, pair_j, count, sums, 1, 0)
    assert count.cpu().numpy()[1:].tolist() == [[-1, -1], [-1, -1]]
    assert per["edge"].cpu().numpy()[1:].tolist() == [0, 0] and per["delta"].cpu().numpy()[1:].tolist() == [0.0, 0.0]
    assert per["rho"].cpu().numpy()[1:].tolist() == [-1, -1]           # NaN sums
    ij = edges["ij"].cpu().numpy()
    assert len(ij) <= 1 and (ij >= 0).all() and (ij < n_p).all()
    label, _ = LK.device_components(dev, n_p, edges)
    tree, _ = LK.device_tree(dev, n_p, edges, label)
    assert tree["level"].cpu().numpy().max() <= 1


# ------------------------------------------------------------------ reproducibility
def test_two_runs_are_bitwise_equal():
    g = _golden()
    world, frame = S.crossing_case()
    for w, f, kw in ((g["world_shifted"], g["piece_pose"], {}), (world, frame, {"min_in": 1, "out_ratio": 0})):
        a = LK.link_sync(w, f, origin=ZERO, return_links=True, **kw)
        b = LK.link_sync(w, f, origin=ZERO, return_links=True, **kw)
        for k in SYNC_KEYS + ("cum",):
            _same(a[k], b[k], k)
        for k in LINK_KEYS:
            _same(a["links"][k], b["links"][k], k)
        assert (a["candidates"], a["edges"]) == (b["candidates"], b["edges"])


# ------------------------------------------------------------------ the map
def _assert_same_map(default, device):
    (fa, na), (fb, nb) = default, device
    assert len(fa) == len(fb)
    for p, q in zip(fa, fb):
        assert len(p) == len(q)
        for x, y in zip(p, q):
            _same(x, y, "fused")
    assert set(na) - set(nb) == {"links"} and set(nb) <= set(na)
    for k in nb:
        if k == "carriers":
            assert len(na[k]) == len(nb[k])
            for x, y in zip(na[k], nb[k]):
                _same(x, y, k)
        elif k in ("n_candidates", "n_edges"):
            assert na[k] == nb[k] and isinstance(nb[k], int)
        else:
            _same(na[k], nb[k], k)
    assert nb["n_candidates"] == len(na["links"]["edge"]) and nb["n_edges"] == int(na["links"]["edge"].sum())


def test_fuse_unmatched_on_the_fixture():
    g = _golden()
    args = (g["pieces"], g["piece_pose"], g["poses"])
    default = LK.fuse_unmatched(*args, step=float(g["step"]), return_nodes=True)
    device = LK.fuse_unmatched(*args, step=float(g["step"]), return_nodes=True, device_sync=True)
    _assert_same_map(default, device)
    assert len(device[0]) == 4
    fused, nodes = LK.fuse_unmatched(*args, step=float(g["step"]), return_nodes=True, device_sync=True, return_links=True)
    for k in LINK_KEYS:
        _same(nodes["links"][k], default[1]["links"][k], k)
    only = LK.fuse_unmatched(*args, step=float(g["step"]), device_sync=True)
    assert len(only) == 4 and all(x.tobytes() == y.tobytes() for p, q in zip(only, default[0]) for x, y in zip(p, q))
    assert LK.fuse_unmatched(g["pieces"][:0], g["piece_pose"][:0], g["poses"], device_sync=True) == []


def test_fuse_unmatched_on_a_generated_case():
    pieces, piece_pose, poses, _ = K.make_case(5, BASE, n_poses=8)
    default = LK.fuse_unmatched(pieces, piece_pose, poses, return_nodes=True)
    device = LK.fuse_unmatched(pieces, piece_pose, poses, return_nodes=True, device_sync=True)
    _assert_same_map(default, device)
    assert len(device[0]) >= 2 and (device[1]["sign"] == -1).any()


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


def test_refine_predictions_and_the_example(tmp_path):
    drive = _write_detector_drive(tmp_path)
    model = _zero_head_model()
    gpu_model = model.cuda().eval()
    a = LK.refine_predictions(gpu_model, str(drive), str(tmp_path / "results.json"))
    b = LK.refine_predictions(gpu_model, str(drive), str(tmp_path / "results.json"), device_sync=True)
    assert a["report"] == b["report"] and a["report"]["edges"] >= 6 and a["report"]["clusters_kept"] == 2
    _assert_same_map((a["fused"], a["nodes"]), (b["fused"], b["nodes"]))
    _same(a["pieces"], b["pieces"], "pieces")
    # the example with --device-sync writes the default's map and prints the default's report
    ckpt = tmp_path / "model.pth"
    torch.save(model.state_dict(), ckpt)
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out = subprocess.run([sys.executable, os.path.join(root, "examples", "refine_predictions.py"), str(drive),
                          str(tmp_path / "results.json"), "--checkpoint", str(ckpt), "--out", str(tmp_path / "map.json"),
                          "--device-sync"], capture_output=True, text=True, timeout=300)
    print(out.stdout[-2000:], out.stderr[-2000:])
    assert out.returncode == 0
    F.write_map_json(str(tmp_path / "default.json"), a["fused"], categories=["lane_line"] * len(a["fused"]))
    assert open(tmp_path / "map.json").read() == open(tmp_path / "default.json").read()
    rep = a["report"]
    assert f"{rep['candidates']} candidate pairs, {rep['edges']} edges, {rep['clusters']} clusters" in out.stdout
