"""Paint tracing without a GPU: the oracle (tests/_trace_oracle.py, the rule of
include/pointnet_refine_hip.h "Paint tracing - the rule" in Python ints and floats) against the
independent numpy restatement and against the fixture, the host chain assembly of
pointnet_refine_amd/trace.py against the oracle's, and the rule's behaviour on analytic clouds: the
two painted lanes of _align_cases.paint_frame, asphalt alone, a dashed lane (straight, turned, bent)
and the drive."""
import os

import numpy as np
import pytest

import _align_cases as AC
import _trace_cases as C
import _trace_oracle as O
from make_golden_g21_paint_trace import KW, lines_csr

FLOOR = 20.0                 # between the asphalt's 0-10 and the paint's 40-60


@pytest.mark.parametrize("name", list(C.DESIGNED) + list(C.SEEDED))
def test_oracle_equals_numpy_restatement(name):
    c = C.case(name)
    C.same_bits(C.paint_peaks_np(c["points"], c["slice_offsets"], **c["kw"]), C.expected(name)[0], name)


@pytest.mark.parametrize("name", C.FIXTURE_CASES)
def test_oracle_equals_fixture(golden_dir, name):
    g = np.load(os.path.join(golden_dir, "g21_paint_trace.npz"))
    c = C.case(name)
    peaks, lines, dropped = C.expected(name)
    p = O.params(c["kw"])
    assert np.array_equal(C.bits(g[f"{name}_points"]), C.bits(c["points"]))
    assert np.array_equal(g[f"{name}_slice_offsets"], c["slice_offsets"])
    assert np.array_equal(C.bits(g[f"{name}_kw"]), C.bits(np.array([float(p[k]) for k in KW])))
    C.same_bits({k: g[f"{name}_{k}"] for k in C.KEYS + ("bright_points",)}, peaks, name)
    verts, l_off, sl_off = lines_csr(lines)
    assert np.array_equal(C.bits(g[f"{name}_line_vertices"]), C.bits(verts))
    assert np.array_equal(g[f"{name}_line_offsets"], l_off) and np.array_equal(g[f"{name}_slice_line_offsets"], sl_off)
    assert int(g[f"{name}_lines_dropped"]) == dropped


def test_designed_cases_show_what_they_are_designed_for():
    cells, _, _ = C.expected("cells")
    # one peak per column; the points lost to a border, a non-finite field, |z| > 512 or qi == 0 are not counted
    assert np.diff(cells["peak_offsets"]).tolist() == [1, 1, 1, 1, 2, 1, 1, 1] and int(cells["bright_points"]) == 10
    assert cells["iy"].tolist() == [0, 14, 6, 7, 3, 12, 11, 7, 11]
    assert cells["weight"].tolist()[6:8] == [2, 2 * 4096 * 256]          # rint to even; the clamp, twice
    peaks, _, _ = C.expected("peaks")
    per_slice = np.diff(peaks["peak_offsets"]).reshape(6, 8).sum(axis=1)
    assert per_slice.tolist() == [0, 1, 1, 2, 3, 1]
    assert peaks["iy"].tolist() == [6, 7, 0, 14, 6, 1, 8, 6] and peaks["count"].tolist() == [3] * 8
    nms0, _, _ = C.expected("nms0")
    assert nms0["iy"].tolist() == [14, 15, 0, 1, 7, 8, 9]                # cell ny - 1 is a peak only with nms 0
    links, lines, dropped = C.expected("links")
    assert [len(ls) for ls in lines] == [1, 1, 0, 1, 0, 1, 0, 0, 0] and dropped == 9
    first = links["peak_offsets"][np.arange(9) * 100]
    succ, pred = links["succ"], links["pred"]
    assert succ[first[0]] == first[0] + 1 and links["iy"][first[0] + 1] < links["iy"][first[0] + 2]      # the tie
    assert pred[first[0] + 2] == -1 and succ[first[0] + 2] == -1                                      # not mutual
    assert succ[first[1]] == first[1] + 1 and succ[first[2]] == -1                                    # tol, tol + 1
    assert succ[first[3]] == first[3] + 1 and succ[first[4]] == -1                                    # the gap
    assert lines[5][0][-1, 0] - lines[5][0][0, 0] == 5.0


@pytest.mark.parametrize("name", list(C.DESIGNED) + list(C.SEEDED))
def test_host_chain_assembly_equals_the_oracle(name):
    from pointnet_refine_amd import trace as T
    c = C.case(name)
    peaks, lines, dropped = C.expected(name)
    p = O.params(c["kw"])
    got, n = T.chain_lines(peaks["xyz"], peaks["col"], peaks["succ"], peaks["pred"], len(c["slice_offsets"]) - 1,
                           O.grid_shape(p)[0], p["min_peaks"], p["min_length"])
    C.same_lines(got, lines, name)
    assert n == dropped


def _trace(points, **kw):
    lines, report = O.trace_lines(points, [0, len(points)], intensity_floor=FLOOR, **kw)
    return [np.array(l) for l in lines[0]], report


def _two_lanes(lines, lateral):
    """Exactly two lines; each spans the slice and every vertex lies within the paint of its lane.
    lateral(line) -> the signed offset of every vertex across the lanes' direction."""
    assert len(lines) == 2
    worst = []
    for line, y in zip(lines, AC.LANE_Y):
        assert line[0, 0] < -24.0 and line[-1, 0] > 24.0
        worst.append(float(np.abs(lateral(line) - y).max()))
        # a weighted centroid of points that all lie inside the band cannot leave it
        assert worst[-1] <= AC.PAINT_HALF + 1e-9
    return worst


def test_analytic_frame_gives_its_two_lanes():
    points, _ = AC.paint_frame()
    lines, report = _trace(points)
    print(report, "largest lateral error per lane:", _two_lanes(lines, lambda l: l[:, 1]))
    assert report["lines"] == 2 and report["bright_points"] == 6000


def test_asphalt_alone_gives_no_peak():
    asphalt = AC.paint_cloud(np.random.default_rng(AC.SEED), -25.0, 25.0, paint_per_m=0.0)
    _, report = _trace(asphalt)
    assert report["bright_points"] == 0 and report["peaks"] == 0 and report["lines"] == 0
    # the scope note: with no floor the asphalt's texture is traced
    lines0, _ = O.trace_lines(asphalt, [0, len(asphalt)])
    assert len(lines0[0]) > 0


def test_dashed_lane_straight_turned_and_bent():
    points, _ = AC.paint_frame()
    dashed = C.dashed(points)
    assert len(dashed) < len(points) - 1500                      # three quarters of one lane's paint are gone
    print("straight:", _two_lanes(_trace(dashed)[0], lambda l: l[:, 1]))
    c, s = np.cos(0.1), np.sin(0.1)
    print("turned:", _two_lanes(_trace(C.turned(dashed, 0.1))[0], lambda l: -s * l[:, 0] + c * l[:, 1]))
    k = 1.0 / 200.0
    print("bent:", _two_lanes(_trace(C.bent(dashed, k))[0], lambda l: l[:, 1] - 0.5 * k * l[:, 0] * l[:, 0]))


def test_every_frame_of_the_drive_gives_two_lines():
    points, offsets, _ = C.drive_slices()
    lines, report = O.trace_lines(points, offsets, intensity_floor=FLOOR)
    assert [len(ls) for ls in lines] == [2, 2, 2, 2] and report["lines"] == 8


def test_driver_checks_parameters_without_a_gpu():
    from pointnet_refine_amd import trace as T
    for kw in (dict(cell=0.0), dict(cell=-0.05), dict(cell=0.005), dict(col=0.01), dict(intensity_floor=float("nan")),
               dict(nms=-1), dict(nms=T.MAX_NMS + 1), dict(nms=1.5), dict(min_points=0), dict(min_weight=0),
               dict(max_gap_cols=-1), dict(half_width=0.0), dict(half_width=200.0), dict(table_bytes=0)):
        with pytest.raises(ValueError):
            T._params("paint_peaks", **kw)
    p = T._params("paint_peaks")
    assert (p["nx"], p["ny"]) == (100, 512) == O.grid_shape(O.DEFAULTS)
    assert {k: p[k] for k in O.DEFAULTS if k in p} == {k: v for k, v in O.DEFAULTS.items() if k in p}
