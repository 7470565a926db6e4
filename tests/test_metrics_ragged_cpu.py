"""Host side of the ragged evaluation (pointnet_refine_amd/metrics.py): the vectorised choice of
calibrate_alignments against the loop of calibrate_alignment, the fine grids, the work-item scan
of the ragged sweep against the tiles a per-problem call launches, and evaluate_scenes refusing
to run without a GPU.  The GPU tests are in test_metrics_ragged_gpu.py."""
import numpy as np
import pytest
import torch

import test_metrics_cpu as R

SHAPES = [(1, 1, 1), (256, 512, 16), (257, 513, 17), (300, 1, 5), (255, 511, 15), (1000, 777, 37), (130, 515, 600)]


def _loop_pick(shifts, means, best=float("inf"), off=(0, 0)):
    """The two loops of calibrate_alignment, as written there."""
    for (dx, dy), d in zip(shifts, means):
        if d < best:
            best, off = d, (dx, dy)
    return best, off


def _tables():
    rng = np.random.default_rng(11)
    grid = R.coarse_grid()
    plain = rng.uniform(1.0, 9.0, len(grid))
    ties = plain.copy()
    ties[[17, 40, 399]] = 0.5                                   # three equal minima: the first wins
    nan_mid = plain.copy()
    nan_mid[150:260] = np.nan
    nan_mid[300] = 0.25
    nan_first = plain.copy()
    nan_first[0] = np.nan
    all_nan = np.full(len(grid), np.nan)
    with_inf = np.full(len(grid), np.inf)
    short = rng.uniform(1.0, 9.0, 7)
    return [(grid, plain), (grid, ties), (grid, nan_mid), (grid, nan_first), (grid, all_nan), (grid, with_inf),
            (grid[:7], short), (grid[:1], np.array([np.nan])), (grid[:0], np.zeros(0))]


def _csr(tables):
    off = np.concatenate([[0], np.cumsum([len(m) for _, m in tables])]).astype(np.int64)
    return np.concatenate([s.reshape(-1, 2) for s, _ in tables]), np.concatenate([m for _, m in tables]), off


def test_pick_equals_the_loop():
    from pointnet_refine_amd.metrics import pick_shifts
    tables = _tables()
    shifts, means, off = _csr(tables)
    n = len(tables)
    dist, offset = pick_shifts(shifts, means, off, np.full(n, np.inf), np.zeros((n, 2)))
    for p, (s, m) in enumerate(tables):
        best, o = _loop_pick(s, m)
        assert dist[p] == best and (offset[p, 0], offset[p, 1]) == o, p
    assert dist[1] == 0.5 and tuple(offset[1]) == tuple(R.coarse_grid()[17])
    assert dist[2] == 0.25 and np.isinf(dist[4]) and tuple(offset[4]) == (0, 0) and np.isinf(dist[5])
    # the second stage carries the first choice over: equal means do not replace it, smaller ones do
    rng = np.random.default_rng(12)
    second = []
    for p, (s, m) in enumerate(tables):
        m2 = rng.uniform(0.2, 9.0, len(m))
        if p == 1 and len(m2):
            m2[:] = 0.5                                          # equal to the carried best: not taken
        if p == 3 and len(m2):
            m2[5:9] = np.nan
        second.append((s + 0.1, m2))
    shifts2, means2, off2 = _csr(second)
    dist2, offset2 = pick_shifts(shifts2, means2, off2, dist, offset)
    for p, (s, m) in enumerate(second):
        best, o = _loop_pick(s, m, *_loop_pick(*tables[p]))
        assert dist2[p] == best and (offset2[p, 0], offset2[p, 1]) == o, p
    assert tuple(offset2[1]) == tuple(R.coarse_grid()[17])
    assert dist[1] == 0.5                                        # the inputs are not written to


def test_fine_grids_equal_the_two_aranges():
    from pointnet_refine_amd.metrics import _grid, fine_grids
    chosen = [_loop_pick(s, m)[1] for s, m in _tables()]          # coarse shifts, and (0, 0) where none was chosen
    chosen += [(-20.0, -10.0), (18.0, 9.0), (0.2 * 3, -0.2 * 7)]
    grids = fine_grids(np.array(chosen, dtype=np.float64))
    for (bx, by), got in zip(chosen, grids):
        want = _grid(np.arange(bx - 2.0, bx + 2.0, 0.2), np.arange(by - 1.0, by + 1.0, 0.2))
        assert got.dtype == np.float64 and np.array_equal(got, want), (bx, by)
        assert np.array_equal(got, R.fine_grid(bx, by))
    # off the coarse lattice np.arange may round to another length: the CSR takes it as it comes
    odd = fine_grids(np.array([[0.1 + 0.2, 1e-9]]))[0]
    assert np.array_equal(odd, R.fine_grid(0.1 + 0.2, 1e-9))


def test_work_items_cover_every_tile_once():
    from pointnet_refine_amd.metrics import sweep_item, sweep_work_items
    shapes = SHAPES + SHAPES
    pc, sc = [s[0] for s in shapes], [s[2] for s in shapes]
    off, n_qt = sweep_work_items(pc, sc)
    assert off[0] == 0 and len(off) == len(shapes) + 1
    for p, (n_pred, _, n_shift) in enumerate(shapes):
        qts, sts = -(-n_pred // 256), -(-n_shift // 16)
        assert n_qt[p] == qts and off[p + 1] - off[p] == qts * sts
        assert sweep_item(off, n_qt, off[p]) == (p, 0, 0)
        assert sweep_item(off, n_qt, off[p + 1] - 1) == (p, qts - 1, sts - 1)
        tiles = [sweep_item(off, n_qt, i) for i in range(off[p], off[p + 1])]
        assert sorted(tiles) == [(p, q, s) for q in range(qts) for s in range(sts)]     # the per-problem grid
    # more problems than a 2-D grid has rows: one tile each, item i is problem i
    off, n_qt = sweep_work_items(np.ones(70000), np.ones(70000))
    assert off[-1] == 70000 and sweep_item(off, n_qt, 69999) == (69999, 0, 0) and sweep_item(off, n_qt, 65536) == (65536, 0, 0)
    # a grid past 2^31 items is counted in 64 bits
    off, _ = sweep_work_items([2 ** 31 - 1] * 2, [2 ** 31 - 1] * 2)
    assert off[-1] == 2 * (2 ** 23) * (2 ** 27) and off.dtype == np.int64
    with pytest.raises(ValueError):
        sweep_work_items([1, 0], [1, 1])


def test_scene_groups():
    from pointnet_refine_amd.metrics import scene_groups
    assert scene_groups([5, 5, 5], None) == [(0, 3)] and scene_groups([], 10) == []
    assert scene_groups([5, 5, 5, 30, 1, 9, 1], 10) == [(0, 2), (2, 3), (3, 4), (4, 6), (6, 7)]
    assert scene_groups([0, 0, 12, 0], 10) == [(0, 2), (2, 3), (3, 4)]        # over the budget: alone


def test_ragged_functions_refuse_to_run_without_gpu(monkeypatch):
    from pointnet_refine_amd import metrics
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    with pytest.raises(RuntimeError, match="GPU") as one:
        metrics.evaluate_scene(None, np.zeros((0, 4), np.float32), [])
    with pytest.raises(RuntimeError, match="GPU") as many:
        metrics.evaluate_scenes(None, [(np.zeros((0, 4), np.float32), [])])
    assert str(one.value) == str(many.value)
    with pytest.raises(RuntimeError, match="GPU"):
        metrics.shift_sweep_ragged([np.zeros((4, 3))], [np.zeros((4, 3))], [np.zeros((1, 2))])
    with pytest.raises(RuntimeError, match="GPU"):
        metrics.calibrate_alignments([[np.zeros((2, 3))]], [[np.ones((2, 3))]])
    # problems that never reach the device: the reference's early exit, per problem
    assert metrics.calibrate_alignments([[], [np.zeros((2, 3))]], [[np.ones((2, 3))], []]) == [((0, 0), 999.0)] * 2
    assert metrics.calibrate_alignments([[]], [[np.ones((2, 3))]], return_tables=True) == [((0, 0), 999.0, {})]
