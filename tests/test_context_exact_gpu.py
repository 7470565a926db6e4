"""prh_context_build against the exact restatement of tests/_context_exact.py: which points are
cropped, in which order they are compacted, and which of them a draw returns - by cloud index,
not in distribution.  Inputs and their conditions (empty boundary band, ambiguity cap, zero-class
gap, points per tube) come from the generators of _context_exact.py and are checked without a GPU
in test_context_exact_cpu.py."""
import numpy as np
import pytest
import torch

import _context_exact as X

pytestmark = pytest.mark.gpu


def _build(case, n, seed=0, max_candidates=None, weights=False, cloud=None, dense=None, line=None):
    """build_contexts_resampled on a case's arrays -> numpy (context, counts[, weights])."""
    from pointnet_refine_amd.context import build_contexts_resampled
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).cuda()
    out = build_contexts_resampled(t(case.cloud if cloud is None else cloud), t(case.dense if dense is None else dense),
                                   t(case.line if line is None else line), n, case.radius, case.decay, seed,
                                   max_candidates, weights)
    return tuple(o.cpu().numpy() for o in out)


# ------------------------------------------------------------------ a. crop set and compaction
def _check_crop(case):
    assert len(case.band()) == 0                                   # condition on the inputs
    ctx, counts, w = _build(case, 1, seed=3, weights=True)
    assert ctx.shape == (case.n_lines, 1, 4)
    for l in range(case.n_lines):
        idx = case.crop(l)
        k = len(idx)
        assert int(counts[l]) == k, (case.name, l)
        if k >= 2:       # K > N = 1: all K weights, in candidate order; unique intensities name the points
            assert np.allclose(w[l, :k], case.weights(l), rtol=3e-5, atol=1e-7), (case.name, l)
        assert not w[l, k if k >= 2 else 0:].any(), (case.name, l)
        if k >= 1:                                                 # the one row is a member of the crop set
            assert int(ctx[l, 0, 3]) in set(case.cloud[idx, 3].astype(np.int64)), (case.name, l)


@pytest.mark.parametrize("npts", X.SWEEP_NPTS)
def test_crop_set_and_order_over_cloud_sizes(npts):
    case = X.sweep_case(npts)
    assert len(case.cloud) == npts
    _check_crop(case)


def test_crop_set_and_order_structured_tubes():
    case = X.structured_case()
    _check_crop(case)
    assert len(case.crop(X.STRUCT_ROLES.index("everything"))) == X.STRUCT_NPTS


@pytest.mark.parametrize("nd,m", X.LIMIT_SHAPES)
def test_crop_at_the_limits_of_dense_and_line_points(nd, m):
    _check_crop(X.sweep_case(X.LIMIT_NPTS, nd, m))


def test_dense_and_line_points_over_the_limit_raise():
    case = X.sweep_case(255)
    with pytest.raises(RuntimeError):
        _build(case, 1, dense=np.zeros((2, 257, 3), np.float32))
    with pytest.raises(RuntimeError):
        _build(case, 1, line=np.zeros((2, 65, 3), np.float32))


# ------------------------------------------------------------------ b. / c. the draw, K > N
def _decode(case, rows, l, by_x=False):
    """Cloud indices of the rows of line l; checks the xyz columns on the way."""
    centre = case.centre(l)
    if by_x:
        x = rows[:, 0].astype(np.float64) + centre[0]
        idx = np.abs(x[:, None] - case.cloud[None, :, 0].astype(np.float64)).argmin(1)
    else:
        inv = np.empty(len(case.cloud), dtype=np.int64)
        inv[case.cloud[:, 3].astype(np.int64)] = np.arange(len(case.cloud))
        code = rows[:, 3].astype(np.int64)
        assert np.array_equal(code.astype(np.float32), rows[:, 3]) and code.min() >= 0 and code.max() < len(inv)
        idx = inv[code]
    pts = case.cloud[idx].astype(np.float64)
    tol = X.mean_tolerance(case.line.shape[1], case.line[l], pts[:, :3])
    assert np.abs(rows[:, :3] - (pts[:, :3] - centre)).max() <= tol, (case.name, l)
    assert np.array_equal(rows[:, 3], case.cloud[idx, 3])
    return idx


def _check_without_replacement(case, ctx, counts, seed, n, l, by_x=False):
    cand = case.crop(l)
    assert int(counts[l]) == len(cand) > n
    assert ctx[l].shape == (n, 4)                                  # exactly N rows
    idx = _decode(case, ctx[l], l, by_x)
    assert np.all(np.diff(idx) > 0), (case.name, seed, l)          # distinct, in cloud order
    must, may = X.selection_bounds(case.keys(l, seed), n)
    chosen = set(idx.tolist())
    assert set(cand[must].tolist()) <= chosen, (case.name, seed, l, sorted(set(cand[must].tolist()) - chosen)[:8])
    assert chosen <= set(cand[may].tolist()), (case.name, seed, l, sorted(chosen - set(cand[may].tolist()))[:8])
    return idx


def _check_with_replacement(case, ctx, counts, seed, n, l):
    cand = case.crop(l)
    k = len(cand)
    assert int(counts[l]) == k <= n
    centre = case.centre(l)
    if k == 0:                                                     # zeros minus the centre
        tol = X.mean_tolerance(case.line.shape[1], case.line[l])
        assert np.abs(ctx[l, :, :3] + centre).max() <= tol and not ctx[l, :, 3].any()
        return
    idx = _decode(case, ctx[l], l)
    assert np.array_equal(idx, cand[X.expected_with_replacement(seed, l, k, n)]), (case.name, seed, l)


@pytest.mark.parametrize("seed", X.DRAW_SEEDS)
@pytest.mark.parametrize("K,N", X.DRAW_SHAPES)
def test_draw_without_replacement_is_the_restated_one(K, N, seed):
    case = X.draw_case(K, N)
    ctx, counts = _build(case, N, seed=seed)
    for l in range(4):
        _check_without_replacement(case, ctx, counts, seed, N, l)


def test_line_index_reaches_the_hash():
    """The same line four times: every copy matches the draw restated with its own line index,
    and no two copies return the same points."""
    K, N = 513, 64
    case = X.draw_case(K, N, same_line=True)
    for seed in X.DRAW_SEEDS:
        ctx, counts = _build(case, N, seed=seed)
        got = [tuple(_check_without_replacement(case, ctx, counts, seed, N, l)) for l in range(4)]
        assert len(set(got)) == 4


def test_flat_intensity_draw():
    case = X.flat_case()
    n = case.promise["n"]
    for seed in X.DRAW_SEEDS:
        ctx, counts = _build(case, n, seed=seed)
        for l in range(4):
            _check_without_replacement(case, ctx, counts, seed, n, l, by_x=True)


def test_uniform_fallback_draw():
    case = X.uniform_case()
    n = case.promise["n"]
    assert all(case.weights(l).sum() < 1e-7 for l in range(4))    # an order clear of the 1e-6 switch
    for seed in X.DRAW_SEEDS:
        ctx, counts = _build(case, n, seed=seed)
        for l in range(4):
            _check_without_replacement(case, ctx, counts, seed, n, l)


@pytest.mark.parametrize("n_pos,n_zero", [(400, 300), (100, 500)])
def test_zero_weight_candidates(n_pos, n_zero):
    """Enough positive weights: no zero-weight point is drawn.  Too few: all positive ones, then
    the first zero-weight candidates in cloud order (the kernel's tie rule; numpy's choice refuses
    such an input)."""
    case = X.zero_case(n_pos, n_zero)
    n = case.promise["n"]
    for seed in X.DRAW_SEEDS:
        ctx, counts = _build(case, n, seed=seed)
        for l in range(4):
            idx = _check_without_replacement(case, ctx, counts, seed, n, l)
            cand, zero = case.crop(l), case.weights(l) < X.ZERO_CLASS
            assert int(zero.sum()) == n_zero
            drawn_zero = np.isin(idx, cand[zero])
            if n_pos >= n:
                assert not drawn_zero.any()
            else:
                assert np.array_equal(np.sort(idx), np.sort(np.concatenate([cand[~zero], cand[zero][:n - n_pos]])))


# ------------------------------------------------------------------ d. K <= N
@pytest.mark.parametrize("N", X.REPLACE_N)
def test_draw_with_replacement_is_the_restated_one(N):
    case = X.replace_case(N)
    assert [len(case.crop(l)) for l in range(4)] == case.promise["k"]
    for seed in X.DRAW_SEEDS:
        ctx, counts = _build(case, N, seed=seed)
        for l in range(4):
            _check_with_replacement(case, ctx, counts, seed, N, l)


@pytest.mark.parametrize("N", X.BRANCH_N)
def test_one_point_decides_the_branch(N):
    more, fewer = X.branch_pair(N)
    assert int((more.cloud != fewer.cloud).any(1).sum()) == 4      # one point per lane
    for seed in X.DRAW_SEEDS[:2]:
        ctx, counts = _build(more, N, seed=seed)
        ctx2, counts2 = _build(fewer, N, seed=seed)
        for l in range(4):
            _check_without_replacement(more, ctx, counts, seed, N, l)
            _check_with_replacement(fewer, ctx2, counts2, seed, N, l)


# ------------------------------------------------------------------ e. empty cloud
def test_empty_cloud():
    case = X.sweep_case(255)
    dense, line = np.repeat(case.dense, 2, 0)[:3], np.repeat(case.line, 2, 0)[:3]
    ctx, counts = _build(case, 5, seed=2, cloud=np.zeros((0, 4), np.float32), dense=dense, line=line)
    assert ctx.shape == (3, 5, 4) and not counts.any()
    for l in range(3):
        centre = line[l].astype(np.float64).mean(0)
        assert np.abs(ctx[l, :, :3] + centre).max() <= X.mean_tolerance(32, line[l]) and not ctx[l, :, 3].any()


# ------------------------------------------------------------------ f. the automatic repeat
def test_repeat_with_a_larger_buffer_is_identical():
    from pointnet_refine_amd.context import build_contexts_resampled
    case = X.retry_case()
    n = case.promise["n"]
    t = lambda a: torch.from_numpy(a).cuda()
    args = (t(case.cloud), t(case.dense), t(case.line), n, case.radius, case.decay, 2 ** 40 + 3)
    a, ca = build_contexts_resampled(*args, None)                  # 8192 slots, then the repeat
    b, cb = build_contexts_resampled(*args, 16384)
    assert int(ca[0]) == 9000
    assert torch.equal(a, b) and torch.equal(ca, cb)
    _check_without_replacement(case, a.cpu().numpy(), ca.cpu().numpy(), 2 ** 40 + 3, n, 0)
