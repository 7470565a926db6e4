"""The order contract of the gate backward's BatchNorm partial sums (tests/_gate_recompute_ref.py), and the
proof that the inputs the GPU test uses tell it apart from the two orders an epilogue would produce more
cheaply: without that, bit-equality of the recomputing epilogue with combine_bwd_kernel would prove nothing."""
import numpy as np

from _gate_recompute_ref import (BIG, F, cancelling_block, cancelling_matrix, contract_partials,
                                 lane_interleaved_partials, plain_chain_partials)


def test_patterns_have_three_different_sums():
    v = cancelling_block()
    c, l, p = contract_partials(v)[0], lane_interleaved_partials(v)[0], plain_chain_partials(v)[0]
    assert c.tolist() == [2.0, 2.0, -2.0, 16.0]
    assert l.tolist() == [1.0, 1.0, -1.0, 13.0]
    assert p.tolist() == [0.0, 0.0, 0.0, 0.0]


def test_contract_skips_rows_beyond_p_and_pads_chains_with_zero():
    # P = 2000: the last block has 16 rows, one full chain and three empty ones; P = 2049: one row
    for P in (2000, 2049, 70):
        v = cancelling_matrix(P, 8, seed=P)
        got = contract_partials(v)
        assert got.shape == ((P + 63) // 64, 8)
        last = v[64 * (got.shape[0] - 1):]
        ref = np.zeros(8, F)
        for g in range(4):          # an empty chain adds +0
            c = np.zeros(8, F)
            for row in last[16 * g:16 * g + 16]:
                c = (c + row).astype(F)
            ref = c if g == 0 else (ref + c).astype(F)
        assert np.array_equal(got[-1], ref)


def test_orders_differ_on_the_gpu_tests_inputs():
    v = cancelling_matrix(2000, 64, seed=3)
    c, l, p = contract_partials(v), lane_interleaved_partials(v), plain_chain_partials(v)
    full = slice(0, 2000 // 64)          # blocks that hold whole patterns
    assert np.mean(c[full] != l[full]) > 0.9
    assert np.mean(c[full] != p[full]) > 0.9
    assert np.mean(l[full] != p[full]) > 0.9


def test_weighted_sums_follow_the_same_order():
    # s2 = fma(dy, z, s2) with z a power of two per column: the product is exact, the chain is that of dy * z
    rng = np.random.default_rng(5)
    v = cancelling_matrix(256, 16, seed=4)
    z = np.exp2(rng.integers(-2, 3, size=16)).astype(F)[None, :] * np.where(rng.random((256, 16)) < 0.5, -1, 1).astype(F)
    w = (v * z).astype(F)
    assert np.array_equal(w.astype(np.float64), v.astype(np.float64) * z.astype(np.float64))
    assert np.mean(contract_partials(w) != lane_interleaved_partials(w)) > 0.5
    assert np.mean(contract_partials(w) != plain_chain_partials(w)) > 0.5
    assert float(BIG) == 16777216.0
