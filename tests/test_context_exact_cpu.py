"""No GPU: the restatement of tests/_context_exact.py against the reference-generated fixture, the
reason the kernel's uniform changed, and the conditions every input of
test_context_exact_gpu.py has to meet (checked on the fp64 reference alone)."""
import os

import numpy as np
import pytest

import _context_exact as X
from oracle import context_oracle as O


def test_crop_and_weights_reproduce_the_reference_fixture(golden_dir):
    g = np.load(os.path.join(golden_dir, "g7_context.npz"))
    cloud = g["cloud"]
    for i in range(4):
        radius, decay, n, _ = g[f"cfg{i}"]
        idx = X.crop_indices(cloud, g[f"dense{i}"], radius)
        assert np.array_equal(idx, np.nonzero(g[f"mask{i}"])[0])
        if len(idx) > int(n):
            # the fixture normalised the float32 intensities in float32: a few 2^-24 from the fp64 copies
            assert np.allclose(X.weights64(cloud[idx], g[f"line{i}"], decay), g[f"weights{i}"], rtol=1e-6, atol=0)


def test_hash_is_splitmix64():
    # first outputs of the published splitmix64 generator from state 0 (state += golden gamma per draw)
    assert int(X.mix64(0)) == 0xE220A8397B1DCDAF
    assert int(X.mix64(0x9E3779B97F4A7C15)) == 0x6E789E6AA1B965F4
    h = X.ctx_hash(2 ** 64 - 1, 3, np.array([0, 1, 2 ** 31 + 5]))
    assert h.dtype == np.uint64 and len(set(h.tolist())) == 3
    assert int(X.ctx_hash(2 ** 64 + 7, 1, 9)) == int(X.ctx_hash(7, 1, 9))               # seed mod 2^64
    assert int(X.ctx_hash(7, 1, 9)) == int(X.mix64(X.mix64(7 ^ (1 << 32 | 9))))
    assert int(X.ctx_hash(7, 1, 9)) != int(X.ctx_hash(7, 2, 9))


def test_uniform_is_strictly_inside_the_unit_interval():
    for top in (0, 2 ** 23 - 1):
        u = X.u01(np.uint64(top << 41 | (2 ** 41 - 1)))
        assert u.dtype == np.float32 and 0.0 < float(u) < 1.0
        assert float(u) == (top + 0.5) / 2 ** 23                                          # exact
    assert np.isfinite(-np.log(-np.log(np.float64(X.u01(np.uint64(2 ** 64 - 1))))))
    # the former 24-bit formula: 2^24 - 0.5 is not a float32, the top value rounds to 1.0 -> G = +inf
    assert float(X.u01_24bit(np.uint64(2 ** 64 - 1))) == 1.0
    assert float(X.u01_24bit(np.uint64((2 ** 23 + 1) << 40))) != (2 ** 23 + 1.5) / 2 ** 24


def test_selection_bounds_rule():
    keys = np.array([5.0, 1.0, 3.0, 3.0 - 1e-4, -np.inf, 0.0, -np.inf, -np.inf])
    must, may = X.selection_bounds(keys, 2, eps=1e-4)
    assert must.tolist() == [0] and may.tolist() == [0, 2, 3]                            # 3 and 3 - 1e-4: either
    must, may = X.selection_bounds(keys, 5, eps=1e-4)
    assert must.tolist() == may.tolist() == [0, 1, 2, 3, 5]                              # exactly the finite ones
    must, may = X.selection_bounds(keys, 7, eps=1e-4)
    assert must.tolist() == may.tolist() == [0, 1, 2, 3, 4, 5, 6]                        # -inf: first in order
    assert X.expected_with_replacement(0, 0, 1, 5).tolist() == [0] * 5


def _clean(case):
    assert len(case.band()) == 0, case.name
    assert case.cloud.dtype == np.float32 and len(case.cloud) < 2 ** 24


def _identified(case):
    inten = case.cloud[:, 3]
    assert np.array_equal(np.sort(inten), np.arange(len(inten), dtype=np.float32)), case.name


@pytest.mark.parametrize("npts", X.SWEEP_NPTS)
def test_inputs_cloud_size_sweep(npts):
    case = X.sweep_case(npts)
    assert len(case.cloud) == npts
    _clean(case)
    _identified(case)
    assert np.array_equal(case.crop(0), X.crop_indices(case.cloud, case.dense[0], case.radius))
    assert np.array_equal(case.band(), X.boundary_band(case.cloud, case.dense, case.radius))
    if npts == 1:
        assert len(case.crop(0)) == 1 and len(case.crop(1)) == 0
    else:
        k = len(case.crop(0))
        assert k >= 2 and len(case.crop(1)) >= 2
        # box decoys: many points inside the bent line's bounding box are outside its tube
        lo, hi = case.dense[0].min(0) - case.radius, case.dense[0].max(0) + case.radius
        in_box = np.all((case.cloud[:, :3] >= lo) & (case.cloud[:, :3] <= hi), axis=1)
        assert in_box.sum() >= 3 * k
        if npts > 1000:
            assert len(np.intersect1d(case.crop(0), case.crop(1))) > 0                   # the tubes overlap


def test_inputs_limits():
    for nd, m in X.LIMIT_SHAPES:
        case = X.sweep_case(X.LIMIT_NPTS, nd, m)
        assert case.dense.shape == (2, nd, 3) and case.line.shape == (2, m, 3)
        _clean(case)
        assert len(case.crop(0)) >= 2


def test_inputs_structured_tubes():
    case = X.structured_case()
    _clean(case)
    _identified(case)
    P, last0 = X.STRUCT_NPTS, case.promise["last_block_start"]
    assert len(case.cloud) == P and last0 == 257 * 256 and P - last0 < 256 and (P + 255) // 256 > 256
    crop = {r: case.crop(i) for i, r in enumerate(X.STRUCT_ROLES)}
    assert len(crop["last_block_only"]) >= 2 and crop["last_block_only"].min() >= last0
    blocks = np.unique(crop["first_and_last_block"] // 256)
    assert blocks.tolist() == [0, 257]
    lo, hi = case.dense[1].min(0) - 1.01 * case.radius, case.dense[1].max(0) + 1.01 * case.radius
    in_box = np.all((case.cloud[:, :3] >= lo) & (case.cloud[:, :3] <= hi), axis=1)
    assert np.unique(np.nonzero(in_box)[0] // 256).tolist() == [0, 257]                  # between: box exit
    assert len(crop["empty"]) == 0 and len(crop["everything"]) == P
    both = np.intersect1d(crop["bent"], crop["crossing"])
    assert 0 < len(both) < min(len(crop["bent"]), len(crop["crossing"]))


def _check_draw_inputs(case, n, seeds=X.DRAW_SEEDS):
    _clean(case)
    assert [len(case.crop(l)) for l in range(case.n_lines)] == case.promise["k"], case.name
    for seed in seeds:                                             # the 1 % ambiguity cap, per case
        lines = [l for l in range(case.n_lines) if len(case.crop(l)) > n]
        assert X.ambiguity(case, seed, n) <= 0.01 * len(lines) * n, (case.name, seed)


@pytest.mark.parametrize("K,N", X.DRAW_SHAPES)
def test_inputs_draw_shapes(K, N):
    case = X.draw_case(K, N)
    _identified(case)
    _check_draw_inputs(case, N)
    for l in range(4):
        assert np.abs(case.keys(l, 0)).max() <= 40                                       # where EPS_KEY is derived


def test_inputs_same_line():
    case = X.draw_case(513, 64, same_line=True)
    assert all(np.array_equal(case.dense[0], case.dense[l]) for l in range(4))
    _check_draw_inputs(case, 64)


def test_inputs_flat_and_uniform():
    flat = X.flat_case()
    _check_draw_inputs(flat, flat.promise["n"])
    assert np.all(flat.cloud[:, 3] == 7.0)
    x = np.sort(flat.cloud[:, 0].astype(np.float64))
    assert np.diff(x).min() > 1e-4                                                       # x names the point
    for l in range(4):
        d = O.nearest_distance(flat.cloud[flat.crop(l), :3], flat.line[l])
        assert np.allclose(flat.weights(l), np.exp(-d / flat.decay), rtol=1e-12)
    uni = X.uniform_case()
    _identified(uni)
    _check_draw_inputs(uni, uni.promise["n"])
    for l in range(4):
        assert O.nearest_distance(uni.cloud[uni.crop(l), :3], uni.line[l]).min() >= 0.5
        assert uni.weights(l).sum() < 1e-7


@pytest.mark.parametrize("n_pos,n_zero", [(400, 300), (100, 500)])
def test_inputs_zero_weights(n_pos, n_zero):
    case = X.zero_case(n_pos, n_zero)
    n = case.promise["n"]
    _identified(case)
    _check_draw_inputs(case, n)
    assert n_pos + n_zero > n
    for l in range(4):
        cand = case.crop(l)
        x = O.nearest_distance(case.cloud[cand, :3], case.line[l]) / case.decay
        assert not ((x > 80) & (x < 120)).any()                                          # the gap is clean
        w = case.weights(l)
        zero = w < X.ZERO_CLASS
        assert np.array_equal(zero, x >= 120) and int(zero.sum()) == n_zero
        assert w[~zero].min() > 2.0 ** -126 and w[~zero].sum() >= 1e-5                   # normal fp32, not uniform
        assert np.all(np.float32(np.exp(-x[zero])) == 0)
        assert np.abs(case.keys(l, 1)[~zero]).max() <= 100


def test_inputs_with_replacement_and_branch_pairs():
    for N in X.REPLACE_N:
        case = X.replace_case(N)
        _clean(case)
        _identified(case)
        assert [len(case.crop(l)) for l in range(4)] == [N, N - 1, 1, 0]
    for N in X.BRANCH_N:
        more, fewer = X.branch_pair(N)
        _check_draw_inputs(more, N, X.DRAW_SEEDS[:2])
        _clean(fewer)
        for l in range(4):
            assert len(more.crop(l)) == N + 1 and len(fewer.crop(l)) == N
            assert np.array_equal(np.setdiff1d(more.crop(l), fewer.crop(l)), [more.crop(l)[N // 2]])
    retry = X.retry_case()
    _identified(retry)
    _check_draw_inputs(retry, 1024, (2 ** 40 + 3,))
    assert len(retry.crop(0)) == 9000 > 8192
