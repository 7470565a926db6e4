"""The surface gate of paint tracing without a GPU: the oracle (tests/_trace_surface_oracle.py, the gate of
include/pointnet_refine_hip.h "Paint tracing - the rule: surface gate" in Python floats) on points
designed one per clause, the header and the export, the parameter checks that need no device, and the
defaults that keep the gate off."""
import inspect
import os
import re

import numpy as np
import pytest

import _trace_oracle as O
import _trace_surface_cases as SC
import _trace_surface_oracle as SO

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_designed_points_one_per_clause():
    case, want_off, rows = SC.designed_case()
    res = SO.paint_peaks(case["points"], case["slice_offsets"], case["ground"], **case["kw"])
    for (what, _, off), keep in zip(rows, res["keep"]):
        assert keep == (off is not True), what
    # a point the tracing rule drops first (z = inf, |z| > 512, qi == 0, outside the grid) is not counted
    assert res["off_surface"] == want_off == [5, 1]
    kept = [r[1] for r in rows if r[2] is False]
    assert res["bright_points"] == len(kept) == 7
    # the gate leaves the rule itself alone: the rows it keeps give what the tracing oracle gives for them
    plain = O.paint_peaks(case["points"][np.array(res["keep"])], [0, 10, 11], **{k: v for k, v in case["kw"].items() if k != "band"})
    assert all(res[k] == plain[k] for k in O.PEAK_KEYS + ("bright_points",))
    # as float32 the two one-ulp points fall back onto the band and are kept
    res32 = SO.paint_peaks(SC.as_float32_values(case)["points"], case["slice_offsets"], case["ground"], **case["kw"])
    assert res32["off_surface"] == [3, 1] and res32["bright_points"] == 9


def test_a_narrower_ground_window_puts_points_of_the_trace_grid_off_the_surface():
    case, _, rows = SC.designed_case()
    ground = np.zeros((2, 6, 4))                                 # x in [-3, 3): 6 cells of 1 m
    res = SO.paint_peaks(case["points"], case["slice_offsets"], ground, g_half_length=3.0, **case["kw"])
    gone = [what for (what, _, _), keep in zip(rows, res["keep"]) if not keep]
    assert sum("outside a ground window" in w or w == "the same: x low" for w in gone) == 2
    wide = SO.paint_peaks(case["points"], case["slice_offsets"], np.zeros((2, 8, 4)), **case["kw"])
    assert res["off_surface"][0] == wide["off_surface"][0] + 2


def test_a_negative_floor_keeps_what_the_floor_rule_would_drop():
    """I = -1 with intensity_floor -5 has qi > 0: the gate keeps it on the surface, where "Paint floor -
    the rule: Surface point" wants I >= 0."""
    pts = np.array([[0.5, 0.5, 0.0, -1.0], [0.5, 0.5, 1.0, -1.0]])
    res = SO.paint_peaks(pts, [0, 2], np.zeros((1, 8, 4)), **dict(SC.KW, intensity_floor=-5.0))
    assert res["keep"] == [True, False] and res["off_surface"] == [1] and res["bright_points"] == 1


def test_ragged_case_is_what_it_is_meant_to_be():
    case, res = SC.ragged_case()
    keep = np.array(res["keep"])
    bright = case["points"][:, 3] > 20.0
    print("bright", int(bright.sum()), "off the surface", res["off_surface"], "peaks", len(res["iy"]))
    assert np.diff(case["slice_offsets"]).tolist() == [0, 1, 257, 5000] and res["off_surface"][:2] == [0, 1]
    assert 0.25 * bright.sum() < sum(res["off_surface"]) < 0.45 * bright.sum() and not (~keep & ~bright).any()
    assert len(res["iy"]) > 20 and res["bright_points"] > 500


def test_header_states_the_rule_and_the_export():
    from pointnet_refine_amd import _lib
    header = open(os.path.join(ROOT, "include", "pointnet_refine_hip.h")).read()
    assert "Paint tracing - the rule: surface gate" in header
    for said in ("off_surface", "fabs(z - g) <= band", "bridge deck", "outside the ground window"):
        assert said in re.sub(r"\s*\n \*\s*", " ", header), said
    decl = re.search(r"^int prh_trace_hist_surface\((.*?)\);", header, flags=re.M | re.S).group(1)
    plain = re.search(r"^int prh_trace_hist\((.*?)\);", header, flags=re.M | re.S).group(1)
    norm = lambda t: [" ".join(a.split()) for a in t.split(",")]
    assert norm(decl)[:len(norm(plain)) - 2] == norm(plain)[:-2] and norm(decl)[-2:] == norm(plain)[-2:]
    assert norm(decl)[len(norm(plain)) - 2:-2] == ["double g_half_length", "double g_half_width", "double ground_cell", "int gx",
                                                  "int gy", "const double* ground", "double band", "long long* off_surface"]
    assert "prh_trace_hist_surface" in _lib.EXPORTS


def test_parameters_are_checked_without_a_gpu():
    from pointnet_refine_amd import paintfloor as PF
    from pointnet_refine_amd import trace as T
    pts, off = np.zeros((3, 4)), np.array([0, 3])
    ground = np.zeros((1, 50, 26))
    for band in (-0.01, float("nan"), float("inf")):
        with pytest.raises(ValueError):
            T.paint_peaks(pts, off, ground=ground, band=band)
        with pytest.raises(ValueError):
            T._surface_params("refine_cloud", {"half_length": 25.0, "half_width": 12.8}, band)
    for bad in (np.zeros((2, 50, 26)), np.zeros((1, 50, 25)), np.zeros((50, 26)), np.zeros((1, 26, 50))):
        with pytest.raises(ValueError):
            T.paint_peaks(pts, off, ground=bad)
    with pytest.raises(ValueError):
        T.paint_peaks(pts, off, ground=ground, ground_cell=0.0)
    with pytest.raises(ValueError):
        T.paint_peaks(pts, off, ground=ground, half_width=6.4)   # the table's window is the trace window: (1, 50, 13)
    with pytest.raises(ValueError):
        PF.ground_shape(np.zeros((1, 50, 25)), 1, PF._params("test"), "test")
    PF.ground_shape(ground, 1, PF._params("test"), "test")
    sp = T._surface_params("test", T._params("test", half_length=8.0, half_width=4.0))
    assert (sp["gx"], sp["gy"], sp["band"], sp["ground_cell"]) == (16, 8, 0.15, 1.0) and T.BAND == PF.BAND == 0.15


def test_the_gate_is_off_by_default():
    from pointnet_refine_amd import paintfloor as PF
    from pointnet_refine_amd import trace as T
    sig = inspect.signature(T.refine_cloud).parameters
    assert sig["surface"].default is False and sig["surface_band"].default == PF.BAND
    for f in (T.paint_peaks, T.trace_lines):
        sig = inspect.signature(f).parameters
        assert sig["ground"].default is None and sig["band"].default == PF.BAND and sig["ground_cell"].default == PF.GROUND_CELL
    assert inspect.signature(PF.paint_floor).parameters["ground"].default is None
    assert inspect.signature(PF.resolve).parameters["ground"].default is None
