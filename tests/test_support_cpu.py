"""The host side of cloud support (pointnet_refine_amd/support.py), which needs no GPU: the segment
grid is conservative, the summaries say what their definitions say, the cases the GPU tests compare
exactly hold the oracle's margins, and the GPU entry points refuse to run without a GPU."""
import math

import numpy as np
import pytest
import torch

import _support_cases as C
import _support_oracle as O
from pointnet_refine_amd import support as S


def _cell_lists(grid):
    off, en = grid["cell_offsets"], grid["entries"]
    return lambda c: [tuple(int(v) for v in e) for e in en[off[c]:off[c + 1]]]


def _check_conservative(lines_shifted, pts, radius, cell):
    """Every usable segment within radius of a point (d2 <= r2 by the rule's own arithmetic) is in
    the list of the point's cell; every list is sorted by line, then segment, without repeats."""
    grid = S.segment_grid(lines_shifted, radius, cell)
    off = grid["cell_offsets"]
    assert off.dtype == np.int32 and grid["entries"].dtype == np.int32 and len(off) == grid["nx"] * grid["ny"] + 1
    assert off[0] == 0 and off[-1] == len(grid["entries"]) and (np.diff(off) >= 0).all()
    lists = _cell_lists(grid)
    for c in range(grid["nx"] * grid["ny"]):
        assert lists(c) == sorted(set(lists(c)))
    cums = [O.carrier_cum(v) for v in lines_shifted]
    r2, near = radius * radius, 0
    for p in pts:
        ix, iy = math.floor((p[0] - grid["x0"]) / grid["cell"]), math.floor((p[1] - grid["y0"]) / grid["cell"])
        inside = 0 <= ix < grid["nx"] and 0 <= iy < grid["ny"]
        mine = lists(iy * grid["nx"] + ix) if inside else []
        for l, v in enumerate(lines_shifted):
            if len(v) < 2:
                continue
            for k, d2 in O.project_point(p, v, cums[l])[3].items():
                if d2 <= r2:
                    near += 1
                    assert inside and (l, k) in mine, (p, l, k, d2)
    return grid, near


@pytest.mark.parametrize("radius,cell", [(0.3, 4.0), (1.0, 1.0), (1.0, 64.0), (8.0, 4.0)])
def test_segment_grid_is_conservative(radius, cell):
    lines, cloud = C.shapes_case()
    origin = O.default_origin(lines)
    shifted = [l - origin for l in lines]
    pts = cloud[np.isfinite(cloud).all(1)][:600, :3].astype(np.float64) - origin
    grid, near = _check_conservative(shifted, pts, radius, cell)
    assert near > 100 and grid["cell"] == cell
    # points on the rim of a tube, where only the guard band of the boxes keeps them
    rng = np.random.default_rng(5)
    a, b = shifted[0][0], shifted[0][1]
    e = b - a
    side = np.array([-e[1], e[0], 0.0]) / np.hypot(e[0], e[1])
    rim = np.stack([a + u * e + s * radius * (1.0 - 1e-13) * side for u in rng.uniform(-0.0, 1.0, 40) for s in (-1.0, 1.0)])
    _, near = _check_conservative(shifted, rim, radius, cell)
    assert near >= 40


def test_segment_grid_random_lines_near_zero():
    rng = np.random.default_rng(11)
    lines = [np.cumsum(rng.normal(0.0, 2.0, (n, 3)), axis=0) + rng.uniform(-30, 30, 3) for n in (2, 7, 40, 1, 0)]
    lines.append(np.repeat(lines[1][2:3], 3, axis=0))
    pts = np.concatenate([l[rng.integers(len(l), size=60)] + rng.normal(0.0, 0.4, (60, 3)) for l in lines[:3]])
    grid, near = _check_conservative(lines, pts, 0.5, 3.0)
    assert near > 60
    listed = {tuple(e) for e in grid["entries"].tolist()}
    assert {l for l, _ in listed} == {0, 1, 2}                     # no segment, no entry
    empty = S.segment_grid([np.zeros((0, 3)), lines[3]], 0.5, 3.0)
    assert empty["nx"] == empty["ny"] == 0 and len(empty["entries"]) == 0 and list(empty["cell_offsets"]) == [0]


def test_segment_grid_cap(monkeypatch):
    lines, _ = C.shapes_case()
    origin = O.default_origin(lines)
    far = [lines[0] - origin, lines[0] - origin + [5.0e6, 5.0e6, 0.0]]
    grid = S.segment_grid(far, 0.3, 4.0)
    assert grid["nx"] * grid["ny"] <= S.MAX_CELLS and grid["cell"] >= 2048.0
    monkeypatch.setattr(S, "MAX_CELLS", 16)
    pts = (lines[0][0] - origin) + np.random.default_rng(2).uniform(-1.0, 1.0, (50, 3)) * [30.0, 1.0, 0.3]
    grid, _ = _check_conservative([l - origin for l in lines], pts, 1.0, 1.0)
    assert grid["nx"] * grid["ny"] <= 16 and grid["cell"] > 1.0
    with pytest.raises(ValueError):
        S.segment_grid(far, 0.0, 4.0)
    with pytest.raises(ValueError):
        S.segment_grid([np.array([[0.0, 0.0, 0.0], [np.nan, 1.0, 0.0]])], 0.3, 4.0)


def _acc(rows):
    return np.array(rows, dtype=np.int64).reshape(-1, 8)


def test_derived_arrays_from_a_hand_made_acc():
    q = 65536
    acc = _acc([[4, 2, 2 * 30 * 256, 4 * (q // 10), 4 * (q // 10) ** 2, 2 * 30 * 256 * (q // 10), -2 * q, 0],
                [0, 0, 0, 0, 0, 0, 0, 0],
                [3, 0, 0, 3 * q, 5 * q * q, 0, 3 * q // 2, 0]])
    d = S.derive(acc)
    assert list(d["n"]) == [4, 0, 3] and list(d["n_paint"]) == [2, 0, 0]
    assert d["weight"][0] == 15.0 and d["weight"][2] == 0.0
    assert d["offset"][0] == (q // 10) / q and d["offset_w"][0] == (q // 10) / q and d["spread"][0] == 0.0
    assert d["z"][0] == -0.5 and d["z"][2] == 0.5 and d["offset"][2] == 1.0
    assert abs(d["spread"][2] - math.sqrt(5.0 / 3.0 - 1.0)) < 1e-15
    assert np.isnan(d["offset_w"][2])                               # hits, none of them bright
    for k in ("weight", "offset_w", "offset", "spread", "z"):
        assert np.isnan(d[k][1]), k                                 # the empty node
    big = acc.copy()
    big[1, 0] = 2 ** 22 - 1
    S.derive(big)
    big[1, 0] = 2 ** 22
    with pytest.raises(OverflowError):
        S.derive(big)


def _node_dict(n, n_paint, offsets, step=0.5):
    acc = np.zeros((len(n), 8), dtype=np.int64)
    acc[:, 0], acc[:, 1] = n, n_paint
    return {"acc": acc, "offsets": np.asarray(offsets, dtype=np.int64), "step": step}


def test_marking_attributes():
    solid = [9] * 10
    dashed = [9, 9, 0, 0, 0, 9, 9, 9, 0, 0]
    unsupported = [9] * 4 + [9, 9]
    n = [20] * 10 + [20] * 10 + [20] * 10 + [2, 3, 4, 4, 20, 20] + [20] * 10 + [0] * 3
    paint = solid + dashed + [2] * 10 + unsupported + [9] * 3 + [0] * 7 + [0] * 3
    a = S.marking_attributes(_node_dict(n, paint, [0, 10, 20, 30, 36, 46, 49, 49]))
    assert [x["marking"] for x in a] == ["solid", "dashed", "none", "solid", "unknown", "unknown", "unknown"]
    assert a[0]["painted_share"] == 1.0 and a[0]["runs"] == 1 and a[0]["mean_run_m"] == 5.0 and np.isnan(a[0]["mean_gap_m"])
    assert a[1]["painted_share"] == 0.5 and a[1]["runs"] == 2 and a[1]["mean_run_m"] == 1.25 and a[1]["mean_gap_m"] == 1.5
    assert a[2]["painted_share"] == 0.0 and a[2]["runs"] == 0 and a[2]["supported_share"] == 1.0      # n_paint below 3
    assert a[3]["supported_share"] == 2 / 6 and a[3]["painted_share"] == 1.0         # paint counts on supported nodes only
    assert a[4]["painted_share"] == 0.3 and a[4]["runs"] == 1                        # one run is not a dashed line
    assert np.isnan(a[5]["painted_share"]) and a[5]["supported_share"] == 0.0        # no supported node
    assert a[6]["supported_share"] == 0.0 and np.isnan(a[6]["painted_share"])        # no node at all
    # thresholds are arguments
    b = S.marking_attributes(_node_dict(n, paint, [0, 10, 20, 30, 36, 46, 49, 49]), min_paint_points=2, solid_share=0.4)
    assert [x["marking"] for x in b[:3]] == ["solid", "solid", "solid"]
    # the polylines of one line, as map_support groups them: a run ends with its polyline
    grouped = {"support": _node_dict([20] * 8, [9] * 8, [0, 4, 8]), "polyline_line": np.array([1, 1]), "lines": 2}
    g = S.marking_attributes(grouped)
    assert g[0]["marking"] == "unknown" and g[1]["marking"] == "solid" and g[1]["runs"] == 2 and g[1]["mean_run_m"] == 2.0


def test_map_summary_from_a_hand_made_acc():
    q = 65536
    acc = _acc([[10, 4, 4 * 256 * 25, -10 * q // 8, 10 * (q // 8) ** 2, -4 * 256 * 25 * (q // 8), 10 * q // 4, 0],
                [2, 0, 0, 2 * q // 8, 2 * (q // 8) ** 2, 0, 0, 0],
                [0, 0, 0, 0, 0, 0, 0, 0]])
    s = S._summary(acc, 5)
    assert s["nodes"] == 3 and s["supported"] == 1 and s["supported_share"] == 1 / 3 and s["points"] == 12
    assert s["offset_w_mean"] == -0.125 and s["offset_rms"] == 0.125
    assert abs(s["offset_mean"] - (-8 / 8) / 12) < 1e-15 and abs(s["z_mean"] - 2.5 / 12) < 1e-15
    e = S._summary(acc[2:], 5)
    assert e["points"] == 0 and all(np.isnan(e[k]) for k in ("offset_mean", "offset_rms", "offset_w_mean", "z_mean"))
    flat, owner, n = S._polylines([[np.zeros((3, 3)), np.ones((2, 3))], [], np.zeros((4, 3)), [[0, 0, 0], [1, 1, 1]]])
    assert [len(p) for p in flat] == [3, 2, 4, 2] and list(owner) == [0, 0, 2, 3] and n == 4


@pytest.mark.parametrize("radius", [0.3, 1.0])
@pytest.mark.parametrize("step", [0.5, 0.37])
def test_margins_of_the_exact_cases(step, radius):
    r = C.shapes_oracle(step, radius)
    print(step, radius, len(r["hits"]), "hits, margins:", r["margins"])
    C.assert_margins(r["margins"])
    assert len(r["hits"]) > 900 and r["margins"]["lead"] > 1e-6
    lines, cloud = C.shapes_case()
    assert np.array_equal(r["acc"], O.accumulate(r["hits"], len(r["acc"]), len(cloud)))
    acc, off = O.support_numpy(cloud, lines, step, radius, C.FLOOR)              # the vectorised restatement agrees
    assert np.array_equal(acc, r["acc"]) and np.array_equal(off, r["offsets"])
    for size in C.SIZES[:-1]:                                      # a prefix of the cloud is a prefix of the hits
        part = O.support(cloud[:size], lines, step, radius, C.FLOOR)
        assert np.array_equal(part["acc"], O.accumulate(r["hits"], len(r["acc"]), size))


def test_margins_of_the_fixture(golden_dir):
    import os
    g = np.load(os.path.join(golden_dir, "g17_cloud_support.npz"))
    off = g["line_offsets"]
    lines = [g["line_vertices"][off[l]:off[l + 1]] for l in range(len(off) - 1)]
    want_lines, want_cloud = C.fixture_case()
    assert all(np.array_equal(a, b) for a, b in zip(lines, want_lines)) and np.array_equal(g["cloud"], want_cloud)
    assert os.path.getsize(os.path.join(golden_dir, "g17_cloud_support.npz")) < 200 * 1024
    r = O.support(g["cloud"], lines, float(g["step"]), float(g["radius"]), float(g["intensity_floor"]))
    C.assert_margins(r["margins"])
    assert np.array_equal(r["acc"], g["acc"]) and np.array_equal(r["offsets"], g["node_offsets"])
    assert np.array_equal((g["cloud"][:, 3] * 4) % 1, np.zeros(len(g["cloud"])))     # intensities in quarters


def test_painted_drive_is_painted():
    poses, cloud, lines = C.painted_drive()
    assert cloud.shape == (120000, 4) and cloud.dtype == np.float32 and len(lines) == 3
    bright = cloud[:, 3] >= 40
    assert (cloud[~bright, 3] < 10).all()
    for l in (0, 1):
        assert (bright & (C._distance_xy(cloud[:, :2].astype(np.float64), lines[l]) <= 0.0751)).sum() >= 600
    assert not (bright & (np.abs(cloud[:, 1] - 3.5) < 0.5)).any()


def test_no_cpu_fallback(monkeypatch):
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    lines, cloud = C.shapes_case()
    for call in (lambda: S.node_support(cloud, lines), lambda: S.map_support(cloud, lines)):
        with pytest.raises(RuntimeError, match="needs a GPU"):
            call()


def test_arguments_are_checked_before_the_device():
    lines, cloud = C.shapes_case()
    for kw in ({"step": 0.0}, {"radius": 0.0}, {"radius": 8.5}, {"intensity_floor": float("nan")}):
        with pytest.raises(ValueError):
            S.node_support(cloud, lines, **kw)
