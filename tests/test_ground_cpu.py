"""The ground-lift rule without a GPU: the oracle (_ground_oracle.py, Python ints and floats) against
an independent vectorised numpy restatement on the stored inputs of g18 and on the seeded cases, the
stored results against both, the rule on an analytic road and under a slab, and the host rule of
lift_lines (stations, interpolation over holes, held ends, an all-hole line).

Bounds.  The analytic road is the plane z = -1.7 + 0.02 x + 0.01 y with N(0, 0.02) noise at 100
points / m^2; every station must lie within 0.05 m of the plane.  0.05 m is more than 10 standard
errors of a mean over >= 25 points (0.02 / 5 = 0.004), and one sixth of the context builder's tube
radius (0.3 m), so passing it guarantees populated tubes.  Everything else is compared as bits."""
import os

import numpy as np
import pytest

import _ground_cases as C
import _ground_oracle as O
from pointnet_refine_amd import ground as GR


def _golden(golden_dir):
    return dict(np.load(os.path.join(golden_dir, "g18_ground_lift.npz")))


def _stored_case(g, name):
    r, z_lo, b, n_bins, min_points, num, den = g[f"{name}_kw"]
    kw = {"radius": float(r), "z_lo": float(z_lo), "bin": float(b), "n_bins": int(n_bins), "min_points": int(min_points),
          "peak_share": (int(num), int(den))}
    pts = np.column_stack([g[f"{name}_points"], np.zeros(len(g[f"{name}_points"]))])
    return {"points": pts, "slice_offsets": g[f"{name}_slice_offsets"], "queries": g[f"{name}_queries"],
            "query_offsets": g[f"{name}_query_offsets"], "kw": kw}


def restate(points, slice_offsets, queries, query_offsets, radius=0.5, min_points=5, peak_share=(1, 2), z_lo=-8.0,
            bin=0.0625, n_bins=256):
    """The rule once more, in numpy array operations: one rounding per operation, as the oracle."""
    r2 = np.float64(radius) * np.float64(radius)
    n_q = len(queries)
    out = {"height": np.full(n_q, np.nan), "count": np.zeros(n_q, dtype=np.int32), "hits": np.zeros(n_q, dtype=np.int32),
           "bin": np.full(n_q, -1, dtype=np.int32)}
    for s in range(len(slice_offsets) - 1):
        p = np.asarray(points[slice_offsets[s]:slice_offsets[s + 1]], dtype=np.float64)
        p = p[np.isfinite(p[:, :3]).all(axis=1)]
        for q in range(query_offsets[s], query_offsets[s + 1]):
            dx, dy = p[:, 0] - queries[q, 0], p[:, 1] - queries[q, 1]
            z = p[dx * dx + dy * dy <= r2, 2]
            out["hits"][q] = len(z)
            f = np.floor((z - z_lo) / bin)
            inside = (f >= 0) & (f < n_bins)
            z, b = z[inside], f[inside].astype(np.int64)
            hist = np.bincount(b, minlength=n_bins)
            c3 = np.convolve(hist, [1, 1, 1])[1:-1]
            peak = int(c3.max())
            if peak < min_points:
                continue
            thr = max(min_points, (peak * peak_share[0] + peak_share[1] - 1) // peak_share[1])
            g = int(np.argmax(c3 >= thr))
            rising = np.diff(c3[g:]) > 0
            g += len(rising) if rising.all() else int(np.argmin(rising))
            sel = np.abs(b - g) <= 1
            qz = np.rint(z[sel] * 65536.0).astype(np.int64)
            out["height"][q] = (np.float64(int(qz.sum())) / np.float64(len(qz))) / 65536.0
            out["count"][q], out["bin"][q] = len(qz), g
    return out


def _same_bits(a, b, what):
    for k in C.KEYS:
        assert a[k].dtype == b[k].dtype and np.array_equal(C.bits(a[k]), C.bits(b[k])), (what, k, a[k], b[k])


@pytest.mark.parametrize("name", C.FIXTURE_CASES)
def test_fixture_is_the_oracle_and_the_restatement(golden_dir, name):
    g = _golden(golden_dir)
    c = _stored_case(g, name)
    made = C.case(name)
    for k in ("slice_offsets", "queries", "query_offsets"):
        assert np.array_equal(c[k], made[k]), k
    assert np.array_equal(C.bits(c["points"][:, :3]), C.bits(made["points"][:, :3])) and c["kw"] == dict(
        {"radius": 0.5, "z_lo": -8.0, "bin": 0.0625, "n_bins": 256, "min_points": 5, "peak_share": (1, 2)}, **made["kw"])
    stored = {k: g[f"{name}_{k}"] for k in C.KEYS}
    args = (c["points"], c["slice_offsets"], c["queries"], c["query_offsets"])
    _same_bits(stored, O.ground_heights(*args, **c["kw"]), name)
    _same_bits(stored, restate(*args, **c["kw"]), name)


def test_fixture_holds_the_cases_it_names(golden_dir):
    g = _golden(golden_dir)
    assert os.path.getsize(os.path.join(golden_dir, "g18_ground_lift.npz")) <= os.path.getsize(
        os.path.join(golden_dir, "g17_cloud_support.npz"))
    assert list(g["hits_hits"]) == [0, 4, 5, 5, 5, 10] and list(g["hits_bin"][:3]) == [-1, -1, 99]
    assert np.isnan(g["hits_height"][:2]).all() and list(g["hits_count"][:4]) == [0, 0, 5, 5]   # d2 == r2 counts
    b = g["bins_bin"]
    assert b[1] == -1 and g["bins_hits"][1] == 14           # just outside: hits and nothing else
    assert b[2] == 0 and b[3] == 254 and g["bins_count"][3] == 5     # the top's lower neighbour rounds onto the edge
    assert b[4] == 99 and b[5] == 51 and b[7] == 79         # equal modes: the lowest; a climb of two; 7 >= ceil(13 / 2)
    assert g["bins_height"][6] == -(98304 + 98306 + 98306 + 98308 + 98308 + 98310 + 98310) / 7.0 / 65536.0   # half to even
    assert list(g["params_bin"]) == [19, 4, -1] and list(g["cells_count"][1:5]) == [63, 64, 65, 257]


@pytest.mark.parametrize("name", ["queries1", "queries5", "queries65", "ragged"])
def test_oracle_is_the_restatement_on_seeded_cases(name):
    c = C.case(name)
    _same_bits(C.expected(name), restate(c["points"], c["slice_offsets"], c["queries"], c["query_offsets"], **c["kw"]), name)
    if name == "ragged":
        e, qo = C.expected(name), c["query_offsets"]
        for s, z in enumerate((-1.7, -0.4, 2.0)):           # every slice finds its own road, not its neighbour's
            assert np.abs(e["height"][qo[s]:qo[s + 1]] - z).max() <= 0.05
        assert np.isnan(e["height"][qo[4]:qo[5]]).all() and (e["hits"][qo[4]:qo[5]] == 0).all()
    elif name != "queries1":
        assert C.expected(name)["hits"][-1] == 0            # the query outside the points' extent


def test_analytic_road_within_5_cm():
    c, plane = C.analytic_road()
    e = O.ground_heights(c["points"], c["slice_offsets"], c["queries"], c["query_offsets"])
    err = np.abs(e["height"] - plane)
    print(f"analytic road: max |height - plane| {err.max():.4f} m, fewest points {e['count'].min()}")
    assert e["count"].min() >= 25
    assert err.max() <= 0.05


def test_road_under_a_slab():
    lower = O.ground_heights(**{k: v for k, v in C.slab_case(1.5).items() if k != "kw"})
    upper = O.ground_heights(**{k: v for k, v in C.slab_case(3.0).items() if k != "kw"})
    print("slab at 1.5x:", lower["height"], "at 3x:", upper["height"])
    assert np.abs(lower["height"] + 1.7).max() <= 0.05      # 1.5 x the road's points above it: the road wins
    assert np.abs(upper["height"] + 0.5).max() <= 0.05      # 3 x: the slab wins, the documented limit


def test_line_stations_and_host_lift(golden_dir):
    g = _golden(golden_dir)
    lo = g["line_offsets"]
    lines = [g["line_vertices"][lo[l]:lo[l + 1]] for l in range(len(lo) - 1)]
    xy, arc, off = GR.line_stations(lines, 1.0)
    assert np.array_equal(off, g["station_offsets"])
    assert np.array_equal(C.bits(arc), C.bits(g["station_arc"])) and np.array_equal(C.bits(xy), C.bits(g["station_xy"]))
    # the bend is 5 + 5.5 + 7.25 = 17.75 m long: stations 0 .. 17 and the end; short lines keep both ends
    assert list(np.diff(off)) == [19, 2, 1, 1, 0, 7] and arc[off[1] - 1] == 17.75 and arc[off[1] + 1] == 0.625
    assert list(xy[off[2]]) == [2.0, -3.0] and list(xy[off[3]]) == [5.0, 5.0]
    lifted, flags = GR.lift_vertices(lines, arc, off, g["station_height"])
    assert np.array_equal(flags, g["lifted_flags"]) and list(flags) == [True, True, True, True, False, False]
    assert np.array_equal(C.bits(np.concatenate(lifted)), C.bits(g["lifted_vertices"]))
    h = g["station_height"]
    z = lifted[0][:, 2]
    assert z[0] == h[2] and z[-1] == h[off[1] - 2]          # the ends hold the first and last valid station
    assert z[1] == h[5] and abs(z[2] - (h[10] + 0.5 * (h[11] - h[10]))) <= 1e-15    # vertices at arc 5 and 10.5
    assert np.array_equal(lifted[5], lines[5]) and lifted[5] is not lines[5]         # all holes: unchanged
    for a, b in zip(lifted, lines):
        assert np.array_equal(a[:, :2], b[:, :2])           # x and y are never changed


def test_validation_and_no_cpu_fallback():
    import torch
    for kw in ({"radius": 0.0}, {"radius": 4.5}, {"n_bins": 257}, {"n_bins": 0}, {"min_points": 0}, {"bin": 0.0},
               {"peak_share": (3, 2)}, {"peak_share": (0, 2)}, {"z_lo": -300.0}, {"z_lo": 250.0}):
        with pytest.raises(ValueError):
            GR._params(**dict({"radius": 0.5, "min_points": 5, "peak_share": (1, 2), "z_lo": -8.0, "bin": 0.0625,
                               "n_bins": 256, "what": "t"}, **kw))
    with pytest.raises(ValueError):
        GR.line_stations([np.zeros((2, 3))], 0.0)
    if not torch.cuda.is_available():
        with pytest.raises(RuntimeError, match="GPU"):
            GR.ground_heights(np.zeros((1, 4)), [0, 1], np.zeros((1, 2)), [0, 1])
        with pytest.raises(RuntimeError, match="GPU"):
            GR.lift_lines(np.zeros((1, 4)), [0, 1], [[np.zeros((2, 3))]])


def test_slice_grids_cover_every_hit():
    """Every hit of the ragged case lies in a cell the query kernel walks: the cells between those of
    q - reach and q + reach, by the kernels' own floor."""
    c = C.case("ragged")
    for cell in (0.5, 2.0):
        gr = GR.slice_grids(c["queries"], c["query_offsets"], 0.5, cell)
        for s in range(len(c["slice_offsets"]) - 1):
            p = c["points"][c["slice_offsets"][s]:c["slice_offsets"][s + 1]]
            for q in c["queries"][c["query_offsets"][s]:c["query_offsets"][s + 1]]:
                hit = p[(p[:, 0] - q[0]) ** 2 + (p[:, 1] - q[1]) ** 2 <= 0.25]
                for d in (0, 1):
                    i = np.floor((hit[:, d] - gr["origin"][s, d]) / gr["cell"])
                    lo = max(np.floor(((q[d] - gr["reach"]) - gr["origin"][s, d]) / gr["cell"]), 0)
                    hi = min(np.floor(((q[d] + gr["reach"]) - gr["origin"][s, d]) / gr["cell"]), gr["shape"][s, d] - 1)
                    assert ((i >= lo) & (i <= hi)).all() and hi - lo <= 3
    assert gr["n_cells"] == int((gr["shape"][:, 0].astype(np.int64) * gr["shape"][:, 1]).sum()) and (gr["shape"][[3, 5]] == 0).all()
