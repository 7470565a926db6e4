"""The paint floor rule without a GPU: the oracle's threshold (tests/_floor_oracle.py) against a
brute-force restatement, the pinned plateau rows, the oracle's gates on the designed points, and the
module's contract (header, exports, RuntimeError without a GPU)."""
import os
import re

import numpy as np
import pytest
import torch

import _align_cases as AC
import _floor_cases as C
import _floor_oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FLOOR_EXPORTS = ["prh_floor_max_bins", "prh_floor_hist", "prh_test_floor_hist", "prh_floor_otsu"]


def test_oracle_equals_brute_force_on_random_small_rows():
    rng = np.random.default_rng(222)
    seen = set()
    for n_bins, min_points in ((2, 1), (3, 1), (7, 4), (16, 16), (33, 1), (40, 30)):
        for h in C.random_rows(rng, 60, n_bins):
            res = O.otsu(h, min_points)
            assert (res["t_lo"], res["t_hi"], res["t"]) == O.otsu_brute(h, min_points), (h, min_points)
            seen.add(res["t"] >= 0)
            seen.add(res["t_hi"] > res["t_lo"])
    assert seen == {True, False}                                 # rows with and without a floor, with and without a plateau


@pytest.mark.parametrize("name", sorted(C.PINNED))
def test_pinned_plateaus(name):
    h, min_points, want = C.PINNED[name]
    res = O.otsu(h, min_points)
    assert (res["t_lo"], res["t_hi"], res["t"]) == want == O.otsu_brute(h, min_points)
    assert res["total"] == sum(h) and res["above"] == sum(h[want[2]:]) and res["score"] > 0.0


def test_paint_drive_intensities_give_10_40_25():
    cloud, _, _ = AC.paint_drive()
    h = [0] * 256
    for v in cloud[:, 3]:
        h[int(v)] += 1
    res = O.otsu(h)
    assert (res["t_lo"], res["t_hi"], res["t"]) == (10, 40, 25)
    share, contrast = O.share_and_contrast(h, res["t"])
    assert abs(share - 0.68) <= 0.02 and 40.0 < contrast < 50.0


@pytest.mark.parametrize("name", sorted(C.NO_FLOOR))
def test_rows_without_a_floor(name):
    h, min_points = C.NO_FLOOR[name]
    res = O.otsu(h, min_points)
    assert (res["t_lo"], res["t_hi"], res["t"], res["above"], res["score"]) == (-1, -1, -1, 0, 0.0)
    assert O.otsu_brute(h, min_points) == (-1, -1, -1)
    if name.startswith("short"):                                 # one more point on the short side: a floor
        b = 3 if name == "short_below" else 30
        assert O.otsu(C.row(64, {3: 16 if b == 3 else 400, 30: 16 if b == 30 else 400}), min_points)["t"] >= 0


def test_isqrt_drive_totals():
    res = O.otsu(C.row(64, {3: 2 ** 40, 40: 2 ** 40}), 16)
    assert (res["t_lo"], res["t_hi"], res["t"]) == (4, 40, 22) and res["wr"] == 2 ** 21 and res["total"] == 2 ** 41


def test_oracle_gates_on_the_designed_points():
    """What the docstring of gates_case says of every point, said by the oracle."""
    c = C.case("gates", 64, 0.5)
    p = O.params(c["kw"])
    got = [O.surface_bin(r, c["ground"][0], p, 8, 4) for r in c["points"][:29]]
    assert got == [2, 3, None, None, None, 6, None, None, None, None, 7, 8, 9, None, None, None, None, None,
                   0, None, None, None, None, 63, 63, 63, 63, 3, 2]
    hist = C.expected("gates", 64, 0.5)
    assert hist.shape == (1, 64) and hist.sum() == sum(b is not None for b in got) + 4 * 64 + 9
    assert hist[0, 63] == 4 + 4 + 9                              # the ladder's last bin and what lies past it


def test_header_states_the_rule_and_the_exports():
    from pointnet_refine_amd import _lib
    header = open(os.path.join(ROOT, "include", "pointnet_refine_hip.h")).read()
    assert "Paint floor - the rule" in header
    declared = re.findall(r"^(?:int|size_t)\s+(prh_(?:test_)?floor_\w+)\(", header, flags=re.M)
    assert declared == FLOOR_EXPORTS and [n for n in _lib.EXPORTS if "floor_" in n] == FLOOR_EXPORTS


@pytest.mark.skipif(torch.cuda.is_available(), reason="the contract without a GPU")
def test_without_a_gpu_it_raises():
    from pointnet_refine_amd import paintfloor as PF
    pts, off = np.zeros((3, 4)), np.array([0, 3])
    for call in (lambda: PF.paint_floor(pts, off), lambda: PF.surface_histograms(pts, off),
                 lambda: PF.surface_ground(pts, off), lambda: PF.otsu_floors(np.zeros((1, 8), dtype=np.int64)),
                 lambda: PF.resolve("auto", pts, off, "test")):
        with pytest.raises(RuntimeError):
            call()


def test_resolve_passes_numbers_and_refuses_the_rest():
    from pointnet_refine_amd import paintfloor as PF
    import pointnet_refine_amd
    assert pointnet_refine_amd.paintfloor is PF
    for v in (0.0, 20, np.float32(3.5)):
        got, report = PF.resolve(v, None, None, "test")
        assert got is v and report is None
    for v in ("Auto", "", None, [20.0], True):
        with pytest.raises(ValueError):
            PF.resolve(v, None, None, "test")
