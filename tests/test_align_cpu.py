"""The paint-alignment rule without a GPU: the oracle (_align_oracle.py, Python ints and floats)
against the independent vectorised numpy restatement (_align_cases.paint_scores_np) on the stored
inputs of g19 and on the seeded cases, the stored results against both, the branches of pick_shift,
the grids, the filter's bitmaps, and the rule on the analytic frame and on the detector drive of
the end-to-end tests.

Bounds.  On the analytic frame and on every frame of the drive the along-lane component of the shift
must be at most 0.02 m (one fine step: the component is unobservable on straight lanes and the rule
returns the shortest near-best shift) and the shifted lines must lie within 0.04 m of the lanes: the
0.02 m near-best bias of the rule's step 9, half a fine step (0.01 m) and 0.01 m for sampling.
Everything else is compared as bits."""
import os

import numpy as np
import pytest

import _align_cases as C
import _align_oracle as O
from pointnet_refine_amd import align as AL


def _golden(golden_dir):
    return dict(np.load(os.path.join(golden_dir, "g19_paint_align.npz")))


def _stored_case(g, name):
    lines = C.from_csr(g[f"{name}_vertices"], g[f"{name}_line_offsets"], g[f"{name}_slice_line_offsets"])
    return {"points": g[f"{name}_points"], "slice_offsets": g[f"{name}_slice_offsets"], "lines": lines,
            "shifts": g[f"{name}_shifts"], "shift_offsets": g[f"{name}_shift_offsets"],
            "kw": {"radius": float(g[f"{name}_kw"][0]), "intensity_floor": float(g[f"{name}_kw"][1])}}


def _args(c):
    return c["points"], c["slice_offsets"], c["lines"], c["shifts"], c["shift_offsets"]


def _same(a, b, what):
    for k in C.KEYS:
        assert a[k].dtype == b[k].dtype == np.int64 and np.array_equal(a[k], b[k]), (what, k, a[k], b[k])


@pytest.mark.parametrize("name", C.FIXTURE_CASES)
def test_stored_cases_oracle_restatement_and_results(golden_dir, name):
    g = _golden(golden_dir)
    c = _stored_case(g, name)
    live = C.case(name)
    for a, b in zip(_args(c)[:2] + _args(c)[3:], _args(live)[:2] + _args(live)[3:]):
        assert np.array_equal(C.bits(a), C.bits(b))           # the generator still gives the stored inputs
    want = {k: g[f"{name}_{k}"] for k in C.KEYS}
    _same(O.paint_scores(*_args(c), **c["kw"]), want, name + " oracle")
    _same(C.paint_scores_np(*_args(c), **c["kw"]), want, name + " restatement")


def test_the_hits_case_holds_what_it_is_designed_for(golden_dir):
    g = _golden(golden_dir)
    c = _stored_case(g, "hits")
    r2 = 0.0625
    line_a, line_c = c["lines"][0][0], c["lines"][0][2]
    assert O.d2_min((1.0, -0.25, 0.0), line_a) == r2                    # d2 == r2 exactly: a hit with qk = 0
    assert O.d2_min((2.0, 0.0, 0.0), line_a) == 0.0 and O.d2_min((2.0, 0.0, 0.0), line_c) == r2
    assert O.d2_min((3.0, float(np.nextafter(-0.25, -np.inf)), 0.0), line_a) > r2
    assert O.d2_min((2.0, 5.0, 0.0), c["lines"][0][1]) == np.inf         # a line of one vertex
    assert O.weight(0.5 / 256.0, 0.0) == 0 and O.weight(1.5 / 256.0, 0.0) == 2 and O.weight(2.5 / 256.0, 0.0) == 2
    assert O.weight(5000.0, 0.0) == 4096 * 256 and O.weight(np.inf, 0.0) == 0 and O.weight(np.nan, 0.0) == 0
    one = O.slice_scores(np.array([[6.0, 0.125, 0.0, 40.0]]), c["lines"][0], [(0.0, 0.0)], r2, 0.0)
    assert one == ([2 * 40 * 256 * 768], [2])                            # in two tubes: (1 - 1/4) * 1024 each
    assert g["hits_hits"][0] >= 8                                        # the designed hitters at shift (0, 0)


@pytest.mark.parametrize("name", sorted(C.SEEDED))
def test_seeded_cases_oracle_against_restatement(name):
    c = C.case(name)
    want = C.expected(name)
    _same(C.paint_scores_np(*_args(c), **c["kw"]), want, name)
    assert want["hits"].sum() > 0
    if name == "segtile":                                                # every designed point hits at shift (0, 0)
        assert list(want["hits"][[0, 2, 4]] >= (4, 4, 5)) == [True, True, True]
    with_floor = O.paint_scores(*_args(c), intensity_floor=20.0) if name == "ragged" else None
    if with_floor is not None:
        _same(C.paint_scores_np(*_args(c), intensity_floor=20.0), with_floor, name + " floor 20")
        assert 0 < with_floor["hits"].sum() < want["hits"].sum()


def test_pick_shift_branches(golden_dir):
    g = _golden(golden_dir)
    sh = g["pick_shifts"]
    for t in range(len(g["pick_score"])):
        got = AL.pick_shift(sh, g["pick_score"][t], g["pick_hits"][t])
        want = O.pick_shift(sh, g["pick_score"][t], g["pick_hits"][t])
        assert np.array_equal(C.bits(got["shift"]), C.bits(g["pick_shift"][t])) and got["aligned"] == bool(g["pick_aligned"][t])
        assert (tuple(got["shift"]), got["aligned"], got["score_zero"], got["score_best"]) == want
    assert g["pick_shift"].tolist() == [[-0.1, 0.0], [-0.1, 0.0], [0.0, 0.0], [0.0, 0.0]]
    assert g["pick_aligned"].tolist() == [True, True, False, False]
    # best == 0
    z = AL.pick_shift(sh, np.zeros(9, dtype=np.int64), np.zeros(9, dtype=np.int64))
    assert not z["aligned"] and z["shift"].tolist() == [0.0, 0.0] and z["row"] == 4
    # min_points decides on the first best row
    few = AL.pick_shift(sh, g["pick_score"][3], g["pick_hits"][3], min_points=31)
    assert few["aligned"] and few["shift"].tolist() == [0.1, 0.1]
    # the gain is strict, and exact in integers far above 2^53
    big = 1 << 60
    assert not AL.pick_shift(sh[3:6], [0, 4 * big, 5 * big], [99] * 3)["aligned"]
    assert AL.pick_shift(sh[3:6], [0, 4 * big, 5 * big + 1], [99] * 3)["aligned"]
    # keep: 63 of 64 is near-best, one less is not
    assert AL.pick_shift(sh[3:9], [0, 1, 64, 0, 63, 0], [99] * 6)["shift"].tolist() == [0.0, 0.1]
    assert AL.pick_shift(sh[3:9], [0, 1, 64, 0, 62, 0], [99] * 6)["shift"].tolist() == [0.0, 0.1]
    assert AL.pick_shift(sh[[8, 5, 4]], [640, 630, 1], [99] * 3)["shift"].tolist() == [0.0, 0.1]
    assert AL.pick_shift(sh[[8, 5, 4]], [640, 629, 1], [99] * 3)["shift"].tolist() == [0.1, 0.1]
    with pytest.raises(ValueError):
        AL.pick_shift(sh[:4], [1] * 4, [99] * 4)               # no (0, 0) row
    for bad in ({"keep": (65, 64)}, {"keep": (0, 64)}, {"gain": (5, 0)}, {"min_points": 0}, {"gain": 1.25}):
        with pytest.raises(ValueError):
            AL.pick_shift(sh, [1] * 9, [99] * 9, **bad)


def test_drive_scope_sums_the_tables():
    """Two slices whose own best rows differ: the drive's pick is the pick of the summed table."""
    sh = O.shift_grid((0.0, 0.0), 0.1, 0.1)
    a = [0, 900, 0, 0, 10, 0, 0, 0, 0]
    b = [0, 0, 0, 0, 10, 0, 0, 2000, 0]
    hits = [40] * 9
    total = AL.pick_shift(sh, [x + y for x, y in zip(a, b)], [2 * h for h in hits])
    assert total["shift"].tolist() == [0.1, 0.0] and AL.pick_shift(sh, a, hits)["shift"].tolist() == [-0.1, 0.0]
    assert AL.pick_shift(sh, b, hits)["shift"].tolist() == [0.1, 0.0]


def test_shift_grid_values():
    g = AL.shift_grid((0.0, 0.0), 1.0, 0.1)
    assert g.shape == (441, 2) and g.dtype == np.float64
    assert g[0].tolist() == [-1.0, -1.0] and g[-1].tolist() == [1.0, 1.0]
    j = np.arange(-10, 11, dtype=np.float64) * 0.1
    assert np.array_equal(C.bits(g[:21, 1]), C.bits(j)) and np.array_equal(C.bits(g[::21, 0]), C.bits(j))
    assert g[220].tolist() == [0.0, 0.0]                       # x outer, y inner: the centre row
    f = AL.shift_grid((0.3, -0.4), 0.1, 0.02)
    assert f.shape == (121, 2) and np.array_equal(C.bits(f), C.bits(O.shift_grid((0.3, -0.4), 0.1, 0.02)))
    assert f[60].tolist() == [0.3, -0.4] and np.array_equal(C.bits(g), C.bits(O.shift_grid((0.0, 0.0), 1.0, 0.1)))
    assert AL.shift_grid((0.0, 0.0), 0.0, 0.1).tolist() == [[0.0, 0.0]]
    assert len(AL.shift_grid((0.0, 0.0), 0.26, 0.1)) == 49     # n = round(2.6) = 3
    with pytest.raises(ValueError):
        AL.shift_grid((0.0, 0.0), 1.0, 0.0)


@pytest.mark.parametrize("name", sorted(C.SEEDED) + list(C.FIXTURE_CASES))
@pytest.mark.parametrize("cell", [0.5, 1.0, 4.0])
def test_segment_bitmaps_are_conservative(name, cell):
    """Every point the oracle counts as a hitter, at any shift of its slice, lies in a set cell."""
    c = C.case(name)
    radius = c["kw"].get("radius", C.RADIUS)
    verts, l_off, sl_off = AL.lines_csr(c["lines"])
    reach = AL.slice_reach(c["shifts"], c["shift_offsets"], radius)
    m = AL.segment_bitmaps(verts, l_off, sl_off, reach, cell)
    assert m["cell"] == cell and m["bitmap"].dtype == np.uint32 and len(m["bitmap"]) == (m["n_cells"] + 31) // 32
    n_hitters = 0
    for s in range(len(sl_off) - 1):
        p = c["points"][c["slice_offsets"][s]:c["slice_offsets"][s + 1]]
        hitters = set()
        O.slice_scores(p, c["lines"][s], c["shifts"][c["shift_offsets"][s]:c["shift_offsets"][s + 1]], radius * radius,
                       0.0, hitters)
        for row in sorted(hitters):
            ix = int(np.floor((p[row, 0] - m["origin"][s, 0]) / m["cell"]))
            iy = int(np.floor((p[row, 1] - m["origin"][s, 1]) / m["cell"]))
            assert 0 <= ix < m["shape"][s, 0] and 0 <= iy < m["shape"][s, 1], (s, row)
            cidx = int(m["cell_base"][s]) + iy * int(m["shape"][s, 0]) + ix
            assert (int(m["bitmap"][cidx >> 5]) >> (cidx & 31)) & 1, (s, row)
        n_hitters += len(hitters)
    assert n_hitters > 0
    # a slice without a vertex has no cell; the far points of `tiles` are in no set cell
    assert all(tuple(m["shape"][s]) == (0, 0) for s in range(len(sl_off) - 1) if l_off[sl_off[s + 1]] == l_off[sl_off[s]])


def test_work_items_cover_every_tile_once():
    items = AL.work_items([0, 0, 257, 300, 301], [0, 16, 33, 50, 51], [3, 3, 0, 3])
    assert items.dtype == np.int64 and items.tolist() == [[1, 0, 16], [1, 256, 16], [1, 0, 32], [1, 256, 32], [3, 300, 50]]


def test_small_frames_align_oracle_against_restatement():
    f = C.small_frames()
    for scope in ("frame", "drive"):
        a = O.align(f["points"], f["slice_offsets"], f["lines"], min_points=8, scope=scope)
        b = O.align(f["points"], f["slice_offsets"], f["lines"], scores=C.paint_scores_np, min_points=8, scope=scope)
        assert np.array_equal(C.bits(a[0]), C.bits(b[0])) and a[1:] == b[1:], scope
        if scope == "frame":
            assert a[1] == [True, False, False]                 # on the paint already: no gain; 5 points: too few
            assert abs(a[0][0, 0]) <= 0.02 and abs(a[0][0, 1] - 0.25) <= 0.04 and a[0][1:].tolist() == [[0.0, 0.0]] * 2
        else:
            assert a[1] == [a[1][0]] * 3 and np.array_equal(a[0][0], a[0][1]) and np.array_equal(a[0][0], a[0][2])


@pytest.mark.parametrize("intensity_floor", [0.0, 20.0])
def test_analytic_frame_within_the_bound(intensity_floor):
    pts, lines = C.paint_frame()
    shifts, aligned, zero, best = O.align(pts, [0, len(pts)], [lines], scores=C.paint_scores_np,
                                          intensity_floor=intensity_floor)
    d = shifts[0]
    along = np.cos(C.YAW) * d[0] + np.sin(C.YAW) * d[1]
    res = C.lateral_residual(lines, d, C.LANE_Y, yaw=C.YAW)
    print(f"floor {intensity_floor}: shift {d.tolist()}, along {along:.4f}, residual {res:.4f}, zero / best {zero[0] / best[0]:.4f}")
    assert aligned == [True]
    assert abs(d[0]) <= C.BOUND_DX and abs(along) <= C.BOUND_DX + 0.5 * C.YAW
    assert res <= C.BOUND_Y
    assert C.lateral_residual(lines, (0.0, 0.0), C.LANE_Y, yaw=C.YAW) > 0.4      # the gap
    assert zero[0] * 5 < best[0]                                # far clearer than the gain asks for


def test_drive_frames_within_the_bound():
    """The generator and seed of test_align_gpu's drive: every frame's own crop of the cloud, through
    the restatement."""
    import _fuse_oracle as FO
    cloud, poses, pixels = C.paint_drive()
    for k, pose in enumerate(poses):
        ego = np.column_stack([FO.to_ego(cloud[:, :3], pose), cloud[:, 3]])
        ego = ego[np.abs(ego[:, 0]) <= 30.0]
        lines = [C.pixel_to_ego(px) for px in pixels[k]]
        shifts, aligned, _, _ = O.align(ego, [0, len(ego)], [lines], scores=C.paint_scores_np)
        res = C.lateral_residual(lines, shifts[0], C.LANE_Y, pose=pose)
        print(f"frame {k}: shift {shifts[0].tolist()}, residual {res:.4f}")
        assert aligned == [True] and abs(shifts[0][0]) <= C.BOUND_DX and res <= C.BOUND_Y
        assert C.lateral_residual(lines, (0.0, 0.0), C.LANE_Y, pose=pose) > 0.4
