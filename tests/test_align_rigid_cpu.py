"""The rigid paint-alignment rule without a GPU: the oracle (_align_rigid_oracle.py, Python ints and
floats) against the independent numpy restatement (_align_rigid_cases.rigid_scores_np) on the stored
inputs of g20 and on the seeded cases; its reduction to the shift rule at theta = 0; the reach and the
filter's bitmaps; pick_pose, pose_grid, pose_table and apply_pose; and the rule on the analytic frame
with the detector's lines turned about the sensor.

Bound of the analytic frame (_align_rigid_cases.BOUND, the rule's step 9'): the shift bias 0.13 r =
0.0195 m, plus the yaw bias 0.13 r sqrt(3) / lever = 1.35 mrad times the 24 m to a line end = 0.0324
m, plus half a fine yaw step times 24 m = 0.012 m: 0.0639 m.  Measured here (floor 20, seed 193):
the shift-only stages leave 0.000 / 0.164 / 0.560 m at 0 / 6 / 15 mrad, the rigid stages 0.000 /
0.026 / 0.028 m.  Everything else is compared as bits."""
import os

import numpy as np
import pytest

import _align_cases as C
import _align_oracle as O
import _align_rigid_cases as RC
import _align_rigid_oracle as RO
from pointnet_refine_amd import align as AL


def _golden(golden_dir):
    return dict(np.load(os.path.join(golden_dir, "g20_paint_align_rigid.npz")))


def _same(a, b, what):
    for k in RC.KEYS:
        assert a[k].dtype == b[k].dtype == np.int64 and np.array_equal(a[k], b[k]), (what, k, a[k], b[k])


@pytest.mark.parametrize("name", RC.FIXTURE_CASES)
def test_stored_cases_oracle_restatement_and_results(golden_dir, name):
    g = _golden(golden_dir)
    live = RC.case(name)
    lines = C.from_csr(g[f"{name}_vertices"], g[f"{name}_line_offsets"], g[f"{name}_slice_line_offsets"])
    for key, now in (("points", live["points"]), ("slice_offsets", live["slice_offsets"]), ("poses", live["poses"]),
                     ("pose_offsets", live["pose_offsets"]), ("pivots", live["pivots"]),
                     ("vertices", C.csr(live["lines"])[0]), ("table", AL.pose_table(live["poses"]))):
        assert np.array_equal(C.bits(g[f"{name}_{key}"]), C.bits(now)), key     # the generator still gives the stored inputs
    a = (g[f"{name}_points"], g[f"{name}_slice_offsets"], lines, g[f"{name}_table"], g[f"{name}_pose_offsets"],
         g[f"{name}_pivots"], float(g[f"{name}_kw"][0]), float(g[f"{name}_kw"][1]))
    want = {k: g[f"{name}_{k}"] for k in RC.KEYS}
    _same(RO.rigid_scores(*a), want, name + " oracle")
    _same(RC.rigid_scores_np(*a), want, name + " restatement")
    _same(RC.rigid_scores_np(*a, chunk=5), want, name + " restatement, chunks of 5")


def test_the_hits_case_holds_what_it_is_designed_for():
    c = RC.case("hits")
    e = RC.expected("hits")
    assert np.array_equal(e["score"][:4], C.expected("hits")["score"]) and np.array_equal(e["hits"][:4], C.expected("hits")["hits"])
    so, ko = c["slice_offsets"], c["pose_offsets"]
    line_a, pivot = c["lines"][1][0], c["pivots"][1]
    table = RO.pose_table(c["poses"][ko[1]:ko[2]])
    pairs = c["points"][so[1]:so[1] + 2 * c["n_boundary_pairs"]]
    for j, row in enumerate((0, 0, 2)):
        (x, y, z, _), (x2, y2, z2, _) = pairs[2 * j], pairs[2 * j + 1]
        assert x == x2 and z == z2 and y2 in (np.nextafter(y, np.inf), np.nextafter(y, -np.inf))
        assert O.d2_min(RO.moved_point(x, y, z, table[row], pivot), line_a) <= 0.0625
        assert O.d2_min(RO.moved_point(x2, y2, z2, table[row], pivot), line_a) > 0.0625
    assert e["hits"][ko[1]:ko[2]].tolist() == [4, 2, 2] and (e["hits"][4:8] > 0).sum() == 3


@pytest.mark.parametrize("name", sorted(RC.SEEDED))
def test_seeded_cases_oracle_against_restatement(name):
    c = RC.case(name)
    want = RC.expected(name)
    got = RC.rigid_scores_np(*RC.args(c)[:3], RO.pose_table(c["poses"]), c["pose_offsets"], c["pivots"], **c["kw"])
    _same(got, want, name)
    assert want["hits"].sum() > 0 and (want["hits"][np.abs(c["poses"][:, 2]) > 0] > 0).any()
    if name == "ragged":
        floor = RC.expected(name, 20.0)
        _same(RC.rigid_scores_np(*RC.args(c)[:3], RO.pose_table(c["poses"]), c["pose_offsets"], c["pivots"],
                                 intensity_floor=20.0), floor, name + " floor 20")
        assert 0 < floor["hits"].sum() < want["hits"].sum()


@pytest.mark.parametrize("name", ["hits", "tiles", "ragged"])
def test_theta_zero_is_the_shift_rule(name):
    """Pivot (0, 0), c = 1, s = 0: _align_oracle.paint_scores' integers."""
    c = C.case(name)
    poses = np.column_stack([c["shifts"], np.zeros(len(c["shifts"]))])
    table = RO.pose_table(poses)
    assert np.array_equal(table[:, 2], np.ones(len(table))) and np.array_equal(table[:, 3], np.zeros(len(table)))
    got = RO.rigid_scores(c["points"], c["slice_offsets"], c["lines"], table, c["shift_offsets"], None, **c["kw"])
    _same(got, C.expected(name), name)
    _same(RC.rigid_scores_np(c["points"], c["slice_offsets"], c["lines"], table, c["shift_offsets"], None, **c["kw"]),
          C.expected(name), name + " restatement")


def test_rigid_reach_values():
    c = RC.case("ragged")
    verts, l_off, sl_off = AL.lines_csr(c["lines"])
    flat = np.column_stack([c["poses"][:, :2], np.zeros(len(c["poses"]))])
    r0 = AL.rigid_reach(flat, c["pose_offsets"], 0.15, verts, l_off, sl_off, c["pivots"])
    assert np.array_equal(C.bits(r0), C.bits(AL.slice_reach(c["poses"][:, :2], c["pose_offsets"], 0.15)))   # a = 0
    r = AL.rigid_reach(c["poses"], c["pose_offsets"], 0.15, verts, l_off, sl_off, c["pivots"])
    assert r.shape == (6,) and np.all(r >= r0) and r[0] > r0[0]
    # slice 0 by hand: line a from the pivot (5, 0.125)
    k0, k1 = c["pose_offsets"][:2]
    m, a = np.abs(c["poses"][k0:k1, :2]).max(), np.abs(c["poses"][k0:k1, 2]).max()
    rho = max(np.sqrt((x - 5.0) * (x - 5.0) + (y - 0.125) * (y - 0.125)) for x, y, _ in c["lines"][0][0])
    assert r[0] == ((0.15 + m) + a * (rho + 0.15)) + 1e-6
    p1 = c["poses"][c["pose_offsets"][1]:c["pose_offsets"][2]]
    assert r[1] == ((0.15 + np.abs(p1[:, :2]).max()) + np.abs(p1[:, 2]).max() * 0.15) + 1e-6    # no vertex: rho = 0


@pytest.mark.parametrize("name", sorted(RC.SEEDED) + list(RC.FIXTURE_CASES))
@pytest.mark.parametrize("cell", [0.5, 1.0, 4.0])
def test_reach_and_bitmaps_are_conservative(name, cell):
    """Every point the oracle counts as a hitter, at any pose of its slice (yaws up to 0.1 rad,
    non-zero pivots), lies in a set cell and inside the reach-expanded box of a segment."""
    c = RC.case(name)
    radius = c["kw"].get("radius", C.RADIUS)
    verts, l_off, sl_off = AL.lines_csr(c["lines"])
    reach = AL.rigid_reach(c["poses"], c["pose_offsets"], radius, verts, l_off, sl_off, c["pivots"])
    m = AL.segment_bitmaps(verts, l_off, sl_off, reach, cell)
    n_hitters = 0
    for s in range(len(sl_off) - 1):
        p = c["points"][c["slice_offsets"][s]:c["slice_offsets"][s + 1]]
        hitters = set()
        RO.slice_scores(p, c["lines"][s], RO.pose_table(c["poses"][c["pose_offsets"][s]:c["pose_offsets"][s + 1]]),
                        c["pivots"][s], radius * radius, 0.0, hitters)
        for row in sorted(hitters):
            ix = int(np.floor((p[row, 0] - m["origin"][s, 0]) / m["cell"]))
            iy = int(np.floor((p[row, 1] - m["origin"][s, 1]) / m["cell"]))
            assert 0 <= ix < m["shape"][s, 0] and 0 <= iy < m["shape"][s, 1], (s, row)
            cidx = int(m["cell_base"][s]) + iy * int(m["shape"][s, 0]) + ix
            assert (int(m["bitmap"][cidx >> 5]) >> (cidx & 31)) & 1, (s, row)
            boxes = [(np.minimum(v[k], v[k + 1])[:2] - reach[s], np.maximum(v[k], v[k + 1])[:2] + reach[s])
                     for v in c["lines"][s] for k in range(len(v) - 1)]
            assert any(lo[0] <= p[row, 0] <= hi[0] and lo[1] <= p[row, 1] <= hi[1] for lo, hi in boxes), (s, row)
        n_hitters += len(hitters)
    assert n_hitters > 0


def test_pose_grid_and_table_values():
    g = AL.pose_grid((0.0, 0.0), 1.0, 0.1, 0.0, 0.02, 0.004)
    assert g.shape == (4851, 3) and g.dtype == np.float64
    assert np.array_equal(C.bits(g), C.bits(RO.pose_grid((0.0, 0.0), 1.0, 0.1, 0.0, 0.02, 0.004)))
    sh = AL.shift_grid((0.0, 0.0), 1.0, 0.1)
    for j in range(11):                                        # the yaw index runs outer
        assert np.array_equal(C.bits(g[441 * j:441 * (j + 1), :2]), C.bits(sh))
        assert np.all(g[441 * j:441 * (j + 1), 2] == (j - 5) * 0.004)
    assert g[441 * 5 + 220].tolist() == [0.0, 0.0, 0.0]
    f = AL.pose_grid((0.3, -0.4), 0.1, 0.02, -0.012, 0.004, 0.001)
    assert f.shape == (1089, 3) and np.array_equal(C.bits(f), C.bits(RO.pose_grid((0.3, -0.4), 0.1, 0.02, -0.012, 0.004, 0.001)))
    one = AL.pose_grid((0.0, 0.0), 1.0, 0.1, 0.0, 0.0, 0.004)
    assert one.shape == (441, 3) and np.array_equal(C.bits(one[:, :2]), C.bits(sh)) and np.all(one[:, 2] == 0.0)
    with pytest.raises(ValueError):
        AL.pose_grid((0.0, 0.0), 1.0, 0.1, 0.0, 0.02, 0.0)
    t = AL.pose_table(f)
    assert t.shape == (1089, 4) and t.flags["C_CONTIGUOUS"] and np.array_equal(C.bits(t), C.bits(RO.pose_table(f)))
    assert AL.pose_table(np.zeros((0, 3))).shape == (0, 4)
    assert AL.pose_table([[1.0, 2.0, 0.0]]).tolist() == [[1.0, 2.0, 1.0, 0.0]]


def _pick(poses, score, hits, **kw):
    got = AL.pick_pose(poses, score, hits, **kw)
    want = RO.pick_pose(poses, score, hits, **kw)
    assert (tuple(got["pose"]), got["aligned"], got["score_zero"], got["score_best"]) == want
    return got


def test_pick_pose_branches():
    ps = AL.pose_grid((0.0, 0.0), 0.1, 0.1, 0.0, 0.004, 0.004)      # 3 yaws x 9 shifts; (0, 0, 0) is row 13
    assert ps.shape == (27, 3) and ps[13].tolist() == [0.0, 0.0, 0.0]
    hits = [40] * 27

    def table(**rows):
        sc = [0] * 27
        sc[13] = 10
        for k, v in rows.items():
            sc[int(k[1:])] = v
        return sc
    # ties go to the lowest row: (-0.1, 0, 0) is row 10, (0.1, 0, 0) row 16, (0, -0.1, 0) row 12
    got = _pick(ps, table(r10=640, r16=640), hits)
    assert got["aligned"] and got["row"] == 10 and got["pose"].tolist() == [-0.1, 0.0, 0.0]
    assert _pick(ps, table(r16=640, r12=640), hits)["row"] == 12
    # the lever norm: (0.1, 0.1, 0) is row 17, 0.02 m^2; (0, 0, 0.004) is row 22, (lever * 0.004)^2
    assert _pick(ps, table(r17=640, r22=640), hits)["row"] == 22                  # 25 m: 0.01 m^2
    assert _pick(ps, table(r17=640, r22=640), hits, lever=50.0)["row"] == 17      # 50 m: 0.04 m^2
    assert _pick(ps, table(r17=640, r22=640), hits, lever=1.0)["pose"].tolist() == [0.0, 0.0, 0.004]
    # keep: 63 of 64 is near-best, one less is not
    assert _pick(ps, table(r17=640, r22=630), hits, lever=25.0)["row"] == 22
    assert _pick(ps, table(r17=640, r22=629), hits, lever=25.0)["row"] == 17
    # best == 0, too few hits at the first best row, no gain
    z = _pick(ps, [0] * 27, [0] * 27)
    assert not z["aligned"] and z["pose"].tolist() == [0.0, 0.0, 0.0] and z["row"] == 13
    few = list(hits)
    few[22] = 31
    assert not _pick(ps, table(r22=9000), few)["aligned"] and _pick(ps, table(r22=9000), few, min_points=31)["aligned"]
    big = 1 << 60
    sc = [0] * 27
    sc[13], sc[22] = 4 * big, 5 * big
    assert not _pick(ps, sc, hits)["aligned"]                   # the gain is strict, and exact far above 2^53
    sc[22] += 1
    assert _pick(ps, sc, hits)["aligned"]
    with pytest.raises(ValueError):
        AL.pick_pose(ps[:13], [1] * 13, [99] * 13)               # no (0, 0, 0) row
    with pytest.raises(ValueError):
        AL.pick_pose(ps[:, :2], [1] * 27, hits)
    for bad in ({"keep": (65, 64)}, {"gain": (5, 0)}, {"min_points": 0}, {"lever": 0.0}, {"lever": np.inf}):
        with pytest.raises(ValueError):
            AL.pick_pose(ps, [1] * 27, hits, **bad)


def test_apply_pose_and_the_rules_inverse():
    rng = np.random.default_rng(7)
    v = np.column_stack([rng.uniform(-30.0, 30.0, 50), rng.uniform(-5.0, 5.0, 50), rng.normal(0.0, 1.0, 50)])
    src = v.copy()
    for pose, pivot in (((0.3, -0.44, 0.015), (0.0, 0.0)), ((-1.0, 0.25, -0.1), (2.0, -1.0)), ((0.0, 0.0, 0.0), (3.0, 3.0))):
        moved = AL.apply_pose(v, pose, pivot)
        assert np.array_equal(v, src) and moved is not v        # the caller's array is not written to
        want = np.array([RO.apply_pose(p, pose, pivot) for p in v])
        assert np.array_equal(C.bits(moved), C.bits(want)) and np.array_equal(moved[:, 2], v[:, 2])
        row = RO.pose_table([pose])[0]
        back = np.array([RO.moved_point(*p, row, pivot) for p in moved])
        assert np.abs(back - v).max() <= 16 * np.finfo(np.float64).eps * 32.0     # a dozen roundings at |coordinate| <= 32
    assert np.array_equal(AL.apply_pose(v, (0.0, 0.0, 0.0)), v)


def test_max_yaw_zero_is_the_shift_procedure():
    f = C.small_frames()
    for scope in ("frame", "drive"):
        a = RO.align(f["points"], f["slice_offsets"], f["lines"], scores=RC.rigid_scores_np, max_yaw=0.0, min_points=8,
                     scope=scope)
        b = O.align(f["points"], f["slice_offsets"], f["lines"], scores=C.paint_scores_np, min_points=8, scope=scope)
        assert np.array_equal(C.bits(a[0][:, :2]), C.bits(b[0])) and np.all(a[0][:, 2] == 0.0) and a[1:] == b[1:], scope


def test_small_frames_align_oracle_against_restatement():
    f = C.small_frames()
    for scope in ("frame", "drive"):
        a = RC.small_align(scope)
        b = RO.align(f["points"], f["slice_offsets"], f["lines"], scores=RC.rigid_scores_np, min_points=8, scope=scope)
        assert np.array_equal(C.bits(a[0]), C.bits(b[0])) and a[1:] == b[1:], scope
        if scope == "frame":
            assert a[1] == [True, False, False] and abs(a[0][0, 1] - 0.25) <= 0.04 and a[0][1:].tolist() == [[0.0] * 3] * 2
        else:
            assert np.array_equal(a[0][0], a[0][1]) and np.array_equal(a[0][0], a[0][2])


@pytest.mark.parametrize("yaw", RC.YAWS)
def test_analytic_frame_within_the_bound(yaw):
    """The detector's lines turned by yaw about the sensor and moved by OFFSET, floor 20, through the
    numpy restatements: what the shift-only stages leave, and what the rigid ones do."""
    pts, lines = RC.yawed_frame(yaw)
    sh, ok, _, _ = O.align(pts, [0, len(pts)], [lines], scores=C.paint_scores_np, intensity_floor=20.0)
    left = RC.lateral_residual(lines, (sh[0][0], sh[0][1], 0.0))
    poses, aligned, zero, best = RO.align(pts, [0, len(pts)], [lines], scores=RC.rigid_scores_np, intensity_floor=20.0)
    res = RC.lateral_residual(lines, poses[0])
    print(f"yaw {yaw}: shift-only {sh[0].tolist()} leaves {left:.4f} m; rigid {poses[0].tolist()} leaves {res:.4f} m "
          f"(bound {RC.BOUND:.4f}), zero / best {zero[0] / best[0]:.4f}")
    assert aligned == [True] and ok == [True]
    assert res <= RC.BOUND
    assert abs(poses[0][0]) <= C.BOUND_DX + 0.44 * yaw          # along-lane: unobservable, none returned but the turn of OFFSET
    if yaw == 0.015:
        assert left > 0.3                                       # a shift cannot take out the rotation
        assert abs(poses[0][2] + yaw) <= 0.13 * C.RADIUS * np.sqrt(3.0) / RC.LEVER + 0.0005
    if yaw == 0.0:
        assert poses[0][2] == 0.0 and np.array_equal(C.bits(poses[0][:2]), C.bits(sh[0]))
