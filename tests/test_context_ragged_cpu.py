"""Host side of the ragged context builder (pointnet_refine_amd.context): the block-offset plan
and the line runs under a byte budget against plain-Python restatements on hand-made inputs, the
argument checks the library makes before it touches a device, the `batched` keyword of the two
end-to-end tools, and the no-CPU-fallback rule."""
import ctypes as C
import inspect

import numpy as np
import pytest
import torch

from pointnet_refine_amd import context as CX


def _block_offsets_plain(slice_offsets, line_slice):
    out = [0]
    for s in line_slice:
        n = slice_offsets[s + 1] - slice_offsets[s]
        out.append(out[-1] + (n + 255) // 256)
    return out


def _runs_plain(cand_offsets, budget):
    """Greedy from the left: a run grows while its candidates fit; a line over the budget runs alone."""
    n = len(cand_offsets) - 1
    room = budget // 8
    runs, l0 = [], 0
    while l0 < n:
        l1 = l0 + 1
        while l1 < n and cand_offsets[l1 + 1] - cand_offsets[l0] <= room:
            l1 += 1
        runs.append((l0, l1))
        l0 = l1
    return runs


# slices of 0, 1, 255, 256, 257, 0, 1000 and 0 points; lines in slices 0 (empty), 2, 2, 3, 4, 4, 4, 6, 7 (empty)
SLICE_OFFSETS = np.cumsum([0, 0, 1, 255, 256, 257, 0, 1000, 0])
LINE_SLICE = [0, 2, 2, 3, 4, 4, 4, 6, 7]


def test_block_offsets_equal_the_restatement():
    got = CX.ragged_block_offsets(SLICE_OFFSETS, LINE_SLICE)
    assert got.dtype == np.int64 and got.tolist() == _block_offsets_plain(SLICE_OFFSETS.tolist(), LINE_SLICE)
    assert got.tolist() == [0, 0, 1, 2, 3, 5, 7, 9, 13, 13]             # by hand: 0 1 1 1 2 2 2 4 0 blocks
    assert CX.ragged_block_offsets([0, 5], []).tolist() == [0]
    rng = np.random.default_rng(3)
    so = np.concatenate(([0], np.cumsum(rng.integers(0, 900, 40) * (rng.random(40) < 0.7))))
    ls = np.sort(rng.integers(0, 40, 300))
    assert CX.ragged_block_offsets(so, ls).tolist() == _block_offsets_plain(so.tolist(), ls.tolist())


@pytest.mark.parametrize("slice_offsets,line_slice", [
    ([0, 4, 9], [1, 0]),            # unsorted
    ([0, 4, 9], [0, 2]),            # slice out of range
    ([0, 4, 9], [-1, 0]),
    ([0, 9, 4], [0, 1]),            # offsets decrease
    ([1, 4, 9], [0, 1]),            # offsets do not start at 0
])
def test_plan_refuses_bad_arguments(slice_offsets, line_slice):
    with pytest.raises(RuntimeError):
        CX.ragged_block_offsets(slice_offsets, line_slice)


def test_line_runs_under_a_budget_equal_the_restatement():
    counts = [0, 10, 0, 300, 5, 5, 0, 0, 120, 1, 0]
    co = np.concatenate(([0], np.cumsum(counts)))
    assert CX.ragged_runs(co, None) == [(0, len(counts))]
    assert CX.ragged_runs([0], None) == [] and CX.ragged_runs([0], 64) == []
    for budget in (0, 7, 8, 80, 8 * 15, 8 * 120, 8 * 130, 8 * 300, 8 * 441, 10 ** 9):
        runs = CX.ragged_runs(co, budget)
        assert runs == _runs_plain(co.tolist(), budget), budget
        assert runs[0][0] == 0 and runs[-1][1] == len(counts) and all(a[1] == b[0] for a, b in zip(runs, runs[1:]))
        for l0, l1 in runs:                              # over the budget only when the run is a single line
            assert (co[l1] - co[l0]) * 8 <= budget or l1 == l0 + 1
    # 80 bytes = 10 candidates: the 300-point line (and the 120-point one) runs alone
    assert (3, 4) in CX.ragged_runs(co, 80) and (8, 9) in CX.ragged_runs(co, 80)
    rng = np.random.default_rng(5)
    co = np.concatenate(([0], np.cumsum(rng.integers(0, 50, 500) * (rng.random(500) < 0.6))))
    for budget in (8, 200, 4000, 10 ** 6):
        assert CX.ragged_runs(co, budget) == _runs_plain(co.tolist(), budget)


def test_library_checks_host_arguments_before_any_device_work():
    """prh_context_ragged_count refuses a bad plan from the host arrays alone (no GPU needed)."""
    from pointnet_refine_amd import _lib
    _lib.build()
    lib = _lib.lib()
    assert lib.prh_context_ragged_workspace_bytes(0, 0) == 0 and lib.prh_context_ragged_workspace_bytes(3, -1) == 0
    assert lib.prh_context_ragged_workspace_bytes(3, 2 ** 31) == 0
    small, large = lib.prh_context_ragged_workspace_bytes(3, 10), lib.prh_context_ragged_workspace_bytes(3, 10 ** 6)
    assert 0 < small < large and large >= 8 * 10 ** 6
    hp = lambda a: a.ctypes.data_as(C.c_void_p)
    fake = C.c_void_p(256)                               # never dereferenced: every case fails a host check first

    def count(so, ls, n_dense=200, radius=0.3):
        so, ls = np.asarray(so, dtype=np.int64), np.asarray(ls, dtype=np.int32)
        seeds = np.zeros(len(so) - 1, dtype=np.uint64)
        return lib.prh_context_ragged_count(fake, hp(so), len(so) - 1, fake, n_dense, hp(ls), hp(seeds), len(ls), radius,
                                            fake, fake, fake, 1 << 20, 0, None)

    for so, ls in (([0, 4, 9], [1, 0]), ([0, 4, 9], [0, 2]), ([0, 4, 9], [-1, 0]), ([0, 9, 4], [0, 1]),
                   ([1, 4, 9], [0, 1]), ([0, 2 ** 31], [0]), ([0, 2 ** 31 - 1], [0] * 300)):
        assert count(so, ls) != 0, (so, ls)
        assert lib.prh_last_error()
    assert count([0, 4, 9], [0, 1], n_dense=257) != 0 and count([0, 4, 9], [0, 1], n_dense=0) != 0
    assert count([0, 4, 9], [0, 1], radius=-1.0) != 0
    so, ls = np.array([0, 4, 9], dtype=np.int64), np.array([0, 1], dtype=np.int32)
    select = lambda m, l0, l1: lib.prh_context_ragged_select(fake, hp(so), 2, fake, 200, fake, m, hp(ls), 2, 0.3, 2.0, 64,
                                                             fake, fake, l0, l1, fake, fake, 100, fake, fake, 1 << 20, 0,
                                                             None)
    assert select(65, 0, 2) != 0 and select(0, 0, 2) != 0               # line points over / under the limits
    assert select(32, 1, 1) != 0 and select(32, 0, 3) != 0 and select(32, -1, 1) != 0


def test_batched_keyword_defaults_to_false():
    from pointnet_refine_amd import fuse, link
    for fn in (fuse.refine_drive, link.refine_predictions):
        assert inspect.signature(fn).parameters["batched"].default is False


def test_no_cpu_fallback():
    pts, dense, line = torch.zeros((10, 4)), torch.zeros((1, 200, 3)), torch.zeros((1, 32, 3))
    with pytest.raises(RuntimeError, match="CUDA"):
        CX.build_contexts_ragged(pts, [0, 10], [np.zeros((2, 3))], [0], [0])
    with pytest.raises(RuntimeError, match="CUDA"):
        CX.build_contexts_ragged_resampled(pts, [0, 10], dense, line, [0], [0])
