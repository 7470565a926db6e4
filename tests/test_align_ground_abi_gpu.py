"""The ground-lift and paint-alignment entry points at the C ABI, through ctypes alone: nothing of align.py or
ground.py is used, so the Python drivers can be rewritten without moving this file.

  prh_ground_bin_count / _write, prh_ground_query
  prh_align_select_count / _write, prh_align_select_cells_count / _write
  prh_align_score, prh_align_score_rigid

Refusals: for every check of every entry, in the order csrc/prh_lib.hip has them, one call that trips that check and
none before it; the return code and the whole text of prh_last_error() are compared.  Every other argument of such a
call is valid (pointers into one zeroed device buffer), so a check that moved or vanished shows as another text, not
as a launch over garbage.

Early exits: the counters start as 0x7f bytes.  A count entry with no point and a non-empty grid zeroes its counters
and nothing behind them; prh_align_select_count zeroes slice_counts even without a cell; the two per-cell count
entries without a cell write nothing; a write entry with capacity 0 takes null outputs.

Direct runs: 2 slices (100 and 30 rows) and 130 points - three waves, the last one partial, the second one holding
rows of both slices - as float64 and as float32: count, torch.cumsum, write, against a numpy restatement of the
kernels' test (finite x y z, floor((x - x0) / cell) in fp64 inside the slice's grid; for align the weight
rint(256 * clamp(I - floor, 0, 4096)) > 0 and the cell's bitmap bit).  Two grids: 'both', where each slice has a grid
and the survivors of the second wave span both slices (the select kernel's per-lane atomics), and 'empty', where
slice 1's grid has shape (0, 0).  Counts are equal; a cell's rows match as a set (ground), a slice's or a cell's
records as a multiset of bytes (align).
"""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

PRH_OK, PRH_ERR_ARG, PRH_ERR_WORKSPACE = 0, -1, -2
NAN, INF = float("nan"), float("inf")

GROUND_GRID = ["points", "is_double", "slice_offsets", "n_slices", "n_points", "origin", "shape", "base", "n_cells", "cell"]
ALIGN_GRID = GROUND_GRID[:8] + ["bitmap", "n_cells", "cell", "floor"]
WRITE = ["offsets", "out", "capacity", "ws", "ws_bytes", "device", "stream"]
SCORE = ["records", "cand_offsets", "n_candidates", "verts", "n_vertices", "line_offsets", "n_lines", "slice_line_offsets",
         "table", "table_offsets", "n_rows"]
SCORE_TAIL = ["reach", "n_slices", "items", "n_items", "r2", "acc", "device", "stream"]
ENTRIES = {
    "ground_bin_count": GROUND_GRID + ["counts", "device", "stream"],
    "ground_bin_write": GROUND_GRID + WRITE,
    "ground_query": GROUND_GRID[:5] + ["queries", "query_offsets", "n_queries"] + GROUND_GRID[5:] + [
        "offsets", "rows", "n_rows", "r2", "reach", "z_lo", "bin", "n_bins", "min_points", "peak_num", "peak_den", "height",
        "count", "hits", "bin_index", "device", "stream"],
    "align_select_count": ALIGN_GRID + ["counts", "device", "stream"],
    "align_select_write": ALIGN_GRID + WRITE,
    "align_select_cells_count": ALIGN_GRID + ["counts", "device", "stream"],
    "align_select_cells_write": ALIGN_GRID + WRITE,
    "align_score": SCORE + SCORE_TAIL,
    "align_score_rigid": SCORE + ["pivots"] + SCORE_TAIL,
}
POINTERS = {"points", "slice_offsets", "origin", "shape", "base", "bitmap", "counts", "offsets", "out", "ws", "queries",
            "query_offsets", "rows", "height", "count", "hits", "bin_index", "records", "cand_offsets", "verts",
            "line_offsets", "slice_line_offsets", "table", "table_offsets", "pivots", "items", "acc"}
# one valid call's scalars; every pointer defaults to the zeroed buffer
SCALARS = {"is_double": 1, "n_slices": 1, "n_points": 1, "n_cells": 1, "cell": 1.0, "floor": 0.0, "capacity": 1,
           "ws_bytes": 256, "n_queries": 1, "n_rows": 1, "r2": 0.0225, "z_lo": -8.0, "bin": 0.0625, "n_bins": 256,
           "min_points": 5, "peak_num": 1, "peak_den": 2, "n_candidates": 1, "n_vertices": 2, "n_lines": 1, "n_items": 1}


def _lib():
    from pointnet_refine_amd import _lib as L
    return L.lib()


@pytest.fixture(scope="module")
def mem():
    """A zeroed, 256-byte aligned device buffer: the address of every pointer a refused call carries."""
    t = torch.zeros((4096,), dtype=torch.uint8, device="cuda")
    assert t.data_ptr() % 256 == 0
    return t


def call(entry, mem, **kw):
    """One call of prh_<entry>: the valid arguments with kw laid over them.  A pointer is given as None, as a byte
    offset into mem, or as a tensor."""
    vals = dict(SCALARS, device=torch.cuda.current_device(),
                stream=C.c_void_p(torch.cuda.current_stream().cuda_stream))
    if entry == "ground_query":
        vals.update(r2=0.25, reach=0.5 + 1e-6)
    vals.update(kw)
    args = []
    for name in ENTRIES[entry]:
        is_ptr = name in POINTERS or (name == "reach" and entry.startswith("align_score"))
        v = vals.get(name, 0 if is_ptr else None)
        if is_ptr and v is not None:
            v = C.c_void_p(v.data_ptr() if torch.is_tensor(v) else mem.data_ptr() + int(v))
        assert v is not None or is_ptr, (entry, name)
        args.append(v)
    return getattr(_lib(), "prh_" + entry)(*args)


def refused(entry, mem, rc, text, **kw):
    got = call(entry, mem, **kw)
    err = _lib().prh_last_error().decode()
    assert (got, err) == (rc, f"{entry}: {text}"), (entry, kw)


def grid_refusals(entry, mem):
    """The checks the grid entries share, in their order."""
    align = entry.startswith("align_")
    bad = "bad argument (at most 2^31 - 1 cells)"
    for kw in ({"n_slices": -1}, {"n_points": -1}, {"n_cells": -1}, {"n_cells": 2 ** 31}, {"n_points": 256 * (2 ** 31 - 1)}):
        refused(entry, mem, PRH_ERR_ARG, bad, **kw)
    for cell in (0.0, -1.0, NAN, INF):
        refused(entry, mem, PRH_ERR_ARG, "cell must be positive and finite", cell=cell)
    if align:
        for floor in (NAN, INF, -INF):
            refused(entry, mem, PRH_ERR_ARG, "intensity_floor must be finite", floor=floor)
    for name in ("slice_offsets", "origin", "shape", "base") + (("bitmap",) if align else ()):
        refused(entry, mem, PRH_ERR_ARG, "null pointer", **{name: None})
    refused(entry, mem, PRH_ERR_ARG, "points without a slice", points=None)
    refused(entry, mem, PRH_ERR_ARG, "points without a slice", n_slices=0)
    if align:
        for is_double, at in ((0, 4), (0, 8), (1, 8)):
            refused(entry, mem, PRH_ERR_ARG, "points must be 16-byte aligned", is_double=is_double, points=at)
    else:
        refused(entry, mem, PRH_ERR_ARG, "points must be aligned to two coordinates (8 bytes)", is_double=0, points=4)
        refused(entry, mem, PRH_ERR_ARG, "points must be aligned to two coordinates (16 bytes)", is_double=1, points=8)
        refused(entry, mem, PRH_ERR_ARG, "points must be aligned to two coordinates (16 bytes)", is_double=1, points=4)
    # the alignment is tested whatever the counts are
    refused(entry, mem, PRH_ERR_ARG, "points must be 16-byte aligned" if align
            else "points must be aligned to two coordinates (16 bytes)", n_slices=0, n_points=0, n_cells=0, points=8)


@pytest.mark.parametrize("entry", ["ground_bin_count", "align_select_count", "align_select_cells_count"])
def test_count_entries_refuse(entry, mem):
    grid_refusals(entry, mem)
    refused(entry, mem, PRH_ERR_ARG, "null pointer", counts=None)


@pytest.mark.parametrize("entry", ["ground_bin_write", "align_select_write", "align_select_cells_write"])
def test_write_entries_refuse(entry, mem):
    lib = _lib()
    grid_refusals(entry, mem)
    refused(entry, mem, PRH_ERR_ARG, "bad capacity", capacity=-1)
    refused(entry, mem, PRH_ERR_ARG, "null pointer", offsets=None)
    refused(entry, mem, PRH_ERR_ARG, "null pointer", out=None)
    if entry != "ground_bin_write":
        refused(entry, mem, PRH_ERR_ARG, "records must be 16-byte aligned", out=8)
    need = {"ground_bin_write": lib.prh_ground_bin_workspace_bytes(3), "align_select_write": lib.prh_align_select_workspace_bytes(3),
            "align_select_cells_write": lib.prh_align_select_cells_workspace_bytes(3)}[entry]
    assert need == 256
    refused(entry, mem, PRH_ERR_WORKSPACE, "workspace too small (256 bytes)", ws=None)
    refused(entry, mem, PRH_ERR_WORKSPACE, "workspace too small (255 bytes)", ws_bytes=255)
    # the size asked for follows the counters: cells for ground and the cell order, slices for the arrival order
    refused(entry, mem, PRH_ERR_WORKSPACE, "workspace too small (256 bytes)",
            **({"n_slices": 65} if entry == "align_select_write" else {"n_cells": 65}))


def test_ground_query_refuses(mem):
    entry = "ground_query"
    grid_refusals(entry, mem)
    for kw in ({"n_queries": -1}, {"n_queries": 4 * (2 ** 31 - 1)}, {"n_rows": -1}, {"n_rows": 2}):
        refused(entry, mem, PRH_ERR_ARG, "bad argument", **kw)
    for kw in ({"r2": 0.0}, {"r2": NAN}, {"r2": 16.5}, {"reach": 0.0}, {"reach": 0.4}, {"reach": 8.5}, {"reach": NAN}):
        refused(entry, mem, PRH_ERR_ARG, "0 < radius <= 4 and radius <= reach <= 8", **kw)
    for kw in ({"n_bins": 0}, {"n_bins": 257}, {"bin": 0.0}, {"bin": NAN}, {"z_lo": -256.5}, {"z_lo": 255.0}):
        refused(entry, mem, PRH_ERR_ARG, "1 <= n_bins <= 256, bin > 0 and the histogram inside [-256, 256]", **kw)
    for kw in ({"min_points": 0}, {"peak_num": 0}, {"peak_num": 3}, {"peak_den": 65537}):
        refused(entry, mem, PRH_ERR_ARG, "min_points >= 1 and 1 <= peak_num <= peak_den <= 65536", **kw)
    for name in ("queries", "query_offsets", "height", "count", "hits", "bin_index", "offsets", "rows"):
        refused(entry, mem, PRH_ERR_ARG, "null pointer", **{name: None})
    assert call(entry, mem, n_queries=0, queries=None, query_offsets=None, height=None, count=None, hits=None,
                bin_index=None, offsets=None, rows=None) == PRH_OK


@pytest.mark.parametrize("entry", ["align_score", "align_score_rigid"])
def test_score_entries_refuse(entry, mem):
    rigid = entry == "align_score_rigid"
    for kw in ({"n_candidates": -1}, {"n_vertices": -1}, {"n_lines": -1}, {"n_rows": -1}, {"n_slices": -1}, {"n_items": -1},
               {"n_items": 2 ** 31}):
        refused(entry, mem, PRH_ERR_ARG, "bad argument (at most 2^31 - 1 work items)", **kw)
    for r2 in (0.0, -1.0, 1.5, NAN):
        refused(entry, mem, PRH_ERR_ARG, "0 < radius <= 1", r2=r2)
    pointers = [n for n in ENTRIES[entry] if n in POINTERS or n == "reach"]
    assert len(pointers) == (11 if rigid else 10)
    for name in pointers:
        refused(entry, mem, PRH_ERR_ARG, "null pointer", **{name: None})
    refused(entry, mem, PRH_ERR_ARG, "null pointer", n_slices=0)
    if rigid:
        refused(entry, mem, PRH_ERR_ARG, "records and poses must be 16-byte aligned", records=8)
        refused(entry, mem, PRH_ERR_ARG, "records and poses must be 16-byte aligned", table=8)
    else:
        refused(entry, mem, PRH_ERR_ARG, "records must be 16-byte aligned", records=8)
    assert call(entry, mem, n_items=0, **{n: None for n in pointers}) == PRH_OK


# ------------------------------------------------------------------ early exits
def _sentinel(n=64):
    return torch.full((n,), 0x7f7f7f7f, dtype=torch.int32, device="cuda")


@pytest.mark.parametrize("entry,counters", [("ground_bin_count", "cells"), ("align_select_count", "slices"),
                                            ("align_select_cells_count", "cells")])
def test_count_without_a_point_zeroes_its_counters(entry, counters, mem):
    counts = _sentinel()
    assert call(entry, mem, n_slices=3, n_cells=5, n_points=0, points=None, counts=counts) == PRH_OK
    n = 5 if counters == "cells" else 3
    got = counts.cpu().numpy()
    assert (got[:n] == 0).all() and (got[n:] == 0x7f7f7f7f).all()


def test_count_without_a_cell(mem):
    counts = _sentinel()
    assert call("align_select_count", mem, n_slices=3, n_cells=0, bitmap=None, counts=counts) == PRH_OK
    got = counts.cpu().numpy()
    assert (got[:3] == 0).all() and (got[3:] == 0x7f7f7f7f).all()          # slice_counts is zeroed all the same
    for entry in ("align_select_cells_count", "ground_bin_count"):
        counts = _sentinel()
        assert call(entry, mem, n_slices=3, n_cells=0, bitmap=None, counts=counts) == PRH_OK
        assert (counts.cpu().numpy() == 0x7f7f7f7f).all()
        assert call(entry, mem, n_slices=3, n_cells=0, bitmap=None, counts=None) == PRH_OK


@pytest.mark.parametrize("entry", ["ground_bin_write", "align_select_write", "align_select_cells_write"])
def test_write_with_capacity_zero_takes_null_outputs(entry, mem):
    assert call(entry, mem, capacity=0, offsets=None, out=None, ws=None, ws_bytes=0) == PRH_OK


# ------------------------------------------------------------------ direct runs
OFF = np.array([0, 100, 130], dtype=np.int64)
CELL, FLOOR = 1.25, 0.25
GRIDS = {"both": np.array([[5, 4], [3, 6]], dtype=np.int32), "empty": np.array([[5, 4], [0, 0]], dtype=np.int32)}
ORIGIN = np.array([[0.25, -0.5], [1.0, 0.5]])


def _cloud(dtype):
    rng = np.random.default_rng(20)
    pts = rng.uniform(-1.0, 7.0, (130, 4))
    pts[:, 3] = rng.uniform(-0.5, 2.0, 130)
    pts[3, 0], pts[70, 1], pts[110, 2], pts[5, 3], pts[120, 3] = NAN, INF, -INF, NAN, INF
    return np.ascontiguousarray(pts.astype(dtype))


def _restated(pts, shape, bitmap_bits):
    """Per point the kernels' test, in fp64: (kept by ground, kept by align, slice, cell, record)."""
    p = pts.astype(np.float64)
    s = np.searchsorted(OFF, np.arange(len(p)), side="right") - 1
    base = np.concatenate([[0], np.cumsum(shape[:, 0].astype(np.int64) * shape[:, 1])[:-1]])
    with np.errstate(invalid="ignore"):
        fx = np.floor((p[:, 0] - ORIGIN[s, 0]) / CELL)
        fy = np.floor((p[:, 1] - ORIGIN[s, 1]) / CELL)
        inside = np.isfinite(p[:, :3]).all(axis=1) & (fx >= 0) & (fx < shape[s, 0]) & (fy >= 0) & (fy < shape[s, 1])
        cell = np.where(inside, base[s] + np.where(inside, fy, 0).astype(np.int64) * shape[s, 0]
                        + np.where(inside, fx, 0).astype(np.int64), 0)
        qi = np.where(np.isfinite(p[:, 3]), np.rint(256.0 * np.clip(p[:, 3] - FLOOR, 0.0, 4096.0)), 0.0).astype(np.int64)
    painted = inside & (qi > 0) & bitmap_bits[cell]
    rec = np.concatenate([np.ascontiguousarray(p[:, :3]).view(np.int64), qi[:, None]], axis=1)        # the record's 32 bytes as four int64
    return inside, painted, s, cell, rec, base


def _setup(dtype, grid):
    shape = GRIDS[grid]
    n_cells = int((shape[:, 0].astype(np.int64) * shape[:, 1]).sum())
    bits = np.random.default_rng(21).random(n_cells) < 0.7
    words = np.zeros(((n_cells + 31) // 32) * 4, dtype=np.uint8)
    packed = np.packbits(bits, bitorder="little")
    words[:len(packed)] = packed
    pts = _cloud(dtype)
    inside, painted, s, cell, rec, base = _restated(pts, shape, bits)
    if grid == "both":                        # the test's own premise: the second wave keeps rows of both slices
        assert set(s[64:128][painted[64:128]]) == {0, 1} and set(s[64:128][inside[64:128]]) == {0, 1}
    else:
        assert not inside[100:].any() and inside[:100].any()
    dev = {k: torch.from_numpy(np.ascontiguousarray(v)).cuda() for k, v in
           {"points": pts, "slice_offsets": OFF, "origin": ORIGIN, "shape": shape, "base": base,
            "bitmap": words.view(np.int32)}.items()}
    kw = dict(dev, is_double=int(dtype == np.float64), n_slices=2, n_points=130, n_cells=n_cells, cell=CELL, floor=FLOOR)
    return kw, inside, painted, s, cell, rec, n_cells


def _count_scan_write(entry, mem, kw, n_counters, out_cols, out_dtype):
    lib = _lib()
    counts = _sentinel(n_counters + 8)
    assert call(entry + "_count", mem, counts=counts, **kw) == PRH_OK, lib.prh_last_error()
    assert (counts[n_counters:].cpu().numpy() == 0x7f7f7f7f).all()
    counts = counts[:n_counters]
    offsets = torch.zeros((n_counters + 1,), dtype=torch.int64, device="cuda")
    offsets[1:] = torch.cumsum(counts, 0)
    total = int(offsets[-1])
    out = torch.zeros((total, out_cols), dtype=out_dtype, device="cuda")
    ws_bytes = getattr(lib, f"prh_{entry}_workspace_bytes")(n_counters)
    ws = torch.empty((ws_bytes,), dtype=torch.uint8, device="cuda")
    assert call(entry + "_write", mem, offsets=offsets, out=out, capacity=total, ws=ws, ws_bytes=ws_bytes, **kw) == PRH_OK, \
        lib.prh_last_error()
    torch.cuda.synchronize()
    return counts.cpu().numpy(), offsets.cpu().numpy(), out.cpu().numpy()


@pytest.mark.parametrize("grid", ["both", "empty"])
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_ground_bin_direct(dtype, grid, mem):
    kw, inside, _, s, cell, _, n_cells = _setup(dtype, grid)
    counts, offsets, rows = _count_scan_write("ground_bin", mem, kw, n_cells, 1, torch.int32)
    assert np.array_equal(counts, np.bincount(cell[inside], minlength=n_cells))
    local = np.arange(130) - OFF[s]
    for c in range(n_cells):
        got = rows[offsets[c]:offsets[c + 1], 0]
        assert len(set(got)) == len(got) and set(got) == set(local[inside & (cell == c)]), c


@pytest.mark.parametrize("grid", ["both", "empty"])
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("entry", ["align_select", "align_select_cells"])
def test_align_select_direct(entry, dtype, grid, mem):
    kw, _, painted, s, cell, rec, n_cells = _setup(dtype, grid)
    key, n = (cell, n_cells) if entry == "align_select_cells" else (s, 2)
    counts, offsets, out = _count_scan_write(entry, mem, kw, n, 4, torch.float64)
    assert np.array_equal(counts, np.bincount(key[painted], minlength=n))
    got = out.view(np.int64)
    for k in range(n):
        want = sorted(r.tobytes() for r in rec[painted & (key == k)])
        assert sorted(r.tobytes() for r in got[offsets[k]:offsets[k + 1]]) == want, k
