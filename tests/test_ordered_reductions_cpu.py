"""The second-stage reductions' order contract without a GPU: the restatement in
_ordered_reductions_ref.py agrees with a plain scalar loop, and - the condition that keeps the GPU
test from passing vacuously - the inputs the GPU test draws tell the contract's order from other
orders.  With plain Gaussian inputs they do not: a reversed or pairwise sum of 256 slabs gives the
same float32 in (nearly) every output."""
import numpy as np
import pytest

import _ordered_reductions_ref as R

OTHER_ORDERS = [R.reversed_order, R.pairwise, R.interleaved2]


def _frac_diff(a, b):
    return float(np.mean(a != b))


def test_seq_is_the_scalar_loop():
    rng = np.random.default_rng(0)
    x = R.gauss(rng, 37, 5)
    for dt in (np.float32, np.float64):
        acc = [dt(0)] * 5
        for t in range(37):
            for c in range(5):
                acc[c] = dt(acc[c] + dt(x[t, c]))
        assert np.array_equal(R.seq(x.astype(dt)), np.array(acc, dt))


def test_fma_is_one_rounding():
    from fractions import Fraction
    rng = np.random.default_rng(1)
    x = rng.standard_normal(2000) ** 2 * 2.0 ** rng.integers(-20, 100, 2000)
    y = rng.integers(1, 129, 2000).astype(np.float64)
    z = rng.standard_normal(2000) * 2.0 ** rng.integers(-20, 100, 2000)
    got = R.fma(x, y, z)
    for i in range(2000):
        q = Fraction(float(x[i])) * Fraction(float(y[i])) + Fraction(float(z[i]))
        assert got[i] == q.numerator / q.denominator


def test_plain_gaussian_inputs_hide_the_order():
    rng = np.random.default_rng(2)
    slab = R.gauss(rng, 256, 20000)
    ref = R.slabs(slab)
    for other in (R.reversed_order, R.pairwise):
        assert _frac_diff(ref, R.slabs(slab, other)) < 0.01


@pytest.mark.parametrize("S", [15, 31, 32, 33, 35, 67, 256])
def test_pairs_show_the_order_slabs(S):
    rng = np.random.default_rng(S)
    slab = R.with_pairs(rng, R.gauss(rng, S, 1000), [np.arange(S)], R.BIG64)
    ref = R.slabs(slab)
    assert np.all(np.isfinite(ref)) and np.abs(ref).max() < 1e3      # the pair itself cancels
    for other in OTHER_ORDERS:
        assert _frac_diff(ref, R.slabs(slab, other)) >= 0.5, other.__name__


def _bn_inputs(rng, Rr, N, ld, pair_a, pair_b, across=False):
    a, b = R.gauss(rng, Rr, ld), np.abs(R.gauss(rng, Rr, ld))
    for groups in R.bn_groups(Rr):
        if pair_a:
            R.with_pairs(rng, a[:, :N], groups, R.BIG64, across)
        if pair_b:
            R.with_pairs(rng, b[:, :N], groups, R.BIG64, across)
    return a, b


def test_pairs_show_the_order_bn_stage1():
    # 8 * 16 * 32 rows: 16 terms per chain in every slice
    rng = np.random.default_rng(3)
    Rr, N = 8 * 16 * 32, 40
    a, b = _bn_inputs(rng, Rr, N, N, True, True)
    ref = R.bn_stage1(a, b, N, 64, Rr * 64, 0)
    for other in OTHER_ORDERS:
        got = R.bn_stage1(a, b, N, 64, Rr * 64, 0, chain=other)
        assert _frac_diff(ref[:, 0], got[:, 0]) >= 0.5 and _frac_diff(ref[:, 1], got[:, 1]) >= 0.5, other.__name__
    # forward: the pair in ws_a shows the order of the sum, the pair in ws_b that of the M2 pass
    a, b = _bn_inputs(rng, Rr, N, N, True, False)
    ref = R.bn_stage1(a, b, N, 64, Rr * 64 - 70, 1)
    for other in OTHER_ORDERS:
        assert _frac_diff(ref[:, 1], R.bn_stage1(a, b, N, 64, Rr * 64 - 70, 1, chain=other)[:, 1]) >= 0.5
    a, b = _bn_inputs(rng, Rr, N, N, False, True)
    ref = R.bn_stage1(a, b, N, 64, Rr * 64 - 70, 1)
    for other in OTHER_ORDERS:
        assert _frac_diff(ref[:, 2], R.bn_stage1(a, b, N, 64, Rr * 64 - 70, 1, chain=other)[:, 2]) >= 0.5
    # the pair across two of the 8 chains: the result is the sum of the chains behind the later
    # one, under the reversed combine that of the chains ahead of the earlier one - the same only
    # when the pair sits in chains 0 and 7 (1 case in 28)
    a, b = _bn_inputs(rng, Rr, N, N, True, True, across=True)
    ref = R.bn_stage1(a, b, N, 64, Rr * 64, 0)
    got = R.bn_stage1(a, b, N, 64, Rr * 64, 0, combine=R.reversed_order)
    assert _frac_diff(ref[:, 0], got[:, 0]) >= 0.5 and _frac_diff(ref[:, 1], got[:, 1]) >= 0.5


def test_pairs_show_the_order_partials():
    rng = np.random.default_rng(4)
    R2, N = 32 * 15, 64
    groups = R.strided_groups(R2, 32)
    a = R.with_pairs(rng, R.gauss(rng, R2, N), groups, R.BIG64)
    b = R.with_pairs(rng, R.gauss(rng, R2, N), groups, R.BIG64)
    ref = R.partials(a, b)
    for other in OTHER_ORDERS:
        got = R.partials(a, b, chain=other)
        assert _frac_diff(ref[0], got[0]) >= 0.5 and _frac_diff(ref[1], got[1]) >= 0.5, other.__name__
    a = R.with_pairs(rng, R.gauss(rng, R2, N), groups, R.BIG64, across=True)
    assert _frac_diff(R.partials(a, None)[0], R.partials(a, None, combine=R.reversed_order)[0]) >= 0.5


def test_pairs_show_the_order_ln_param_grad():
    rng = np.random.default_rng(5)
    nb = 4 * 16 + 2
    groups = R.strided_groups(nb, 4)
    g = R.with_pairs(rng, R.gauss(rng, nb, 256), groups, R.BIG64)
    b = R.with_pairs(rng, R.gauss(rng, nb, 256), groups, R.BIG64)
    ref = R.ln_param_grad(g, b)
    for other in OTHER_ORDERS:
        got = R.ln_param_grad(g, b, chain=other)
        assert _frac_diff(ref[0], got[0]) >= 0.5 and _frac_diff(ref[1], got[1]) >= 0.5, other.__name__
    # across the 4 chains: (0+1)+(2+3) and ((0+1)+2)+3 differ for the pair in chains (2,3), (0,2)
    # and (1,2), 3 of the 6 placements - so about half of the outputs, and at least a quarter
    g = R.with_pairs(rng, R.gauss(rng, nb, 256), groups, R.BIG64, across=True)
    assert _frac_diff(R.ln_param_grad(g, g)[0], R.ln_param_grad(g, g, combine=R.seq)[0]) >= 0.25


def test_pairs_show_the_order_finals():
    rng = np.random.default_rng(6)
    nblk, n_el = 16 * 16 + 3, 387
    groups = R.strided_groups(nblk, 16)
    p = R.with_pairs(rng, R.gauss(rng, nblk, n_el), groups, R.BIG32)
    ref = R.partial_rows_final(p)
    assert np.abs(ref).max() < 1e3
    for other in OTHER_ORDERS:
        assert _frac_diff(ref, R.partial_rows_final(p, chain=other)) >= 0.5, other.__name__
    p = R.with_pairs(rng, R.gauss(rng, nblk, n_el), groups, R.BIG32, across=True)
    assert _frac_diff(R.partial_rows_final(p), R.partial_rows_final(p, combine=R.reversed_order)) >= 0.5
    dw, db = R.pos_hidden_final(p[:, :384])
    assert dw.shape == (96, 3) and db.shape == (96,)
