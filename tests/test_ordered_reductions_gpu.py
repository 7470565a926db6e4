"""The second-stage reduction kernels against the order contract, bit for bit: each raw entry point
(prh_test_reduce_*, which launch through the library's own launchers) must equal the numpy
restatement in _ordered_reductions_ref.py exactly.  The inputs carry a +BIG / -BIG pair per summed
column, which test_ordered_reductions_cpu.py shows tells the contract's order from other orders.
Sizes sit around the depth D of each kernel's load batches: below, at, above, and two batches plus
a remainder."""
import ctypes as C

import numpy as np
import pytest

import _ordered_reductions_ref as R

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

SLABS, BN1, PARTIALS, LN, FINAL, AMAX = range(6)


@pytest.fixture(scope="module")
def lib():
    from pointnet_refine_amd import _lib
    return _lib.lib()


def _dev(x):
    return None if x is None else torch.from_numpy(np.ascontiguousarray(x)).cuda()


def _p(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def _st():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _depth(lib, kind):
    d = lib.prh_test_reduce_depth(kind)
    assert d >= 2
    return d


# ---------------------------------------------------------------- slabs
def _run_slabs(lib, slab, rows, cols, ldout, cslab=None):
    S = slab.shape[0]
    out = torch.full((rows, ldout), -7.0, device="cuda")
    ccols = 0 if cslab is None else cslab.shape[1]
    cout = None if cslab is None else torch.full((ccols,), -7.0, device="cuda")
    ds, dc = _dev(slab), _dev(cslab)
    rc = lib.prh_test_reduce_slabs(_p(ds), S, rows, cols, _p(out), ldout, _p(dc), ccols, _p(cout), 0, _st())
    assert rc == 0, lib.prh_last_error()
    torch.cuda.synchronize()
    out = out.cpu().numpy()
    assert np.all(out[:, cols:] == -7.0)                    # the pad columns of ldout stay untouched
    return out[:, :cols], None if cout is None else cout.cpu().numpy()


def _slab_inputs(rng, S, n):
    return R.with_pairs(rng, R.gauss(rng, S, n), [np.arange(S)], R.BIG64)


def test_slabs_depth_edges(lib):
    D = _depth(lib, SLABS)
    rng = np.random.default_rng(10)
    for S in (1, D - 1, D, D + 1, 2 * D + 3):
        slab = _slab_inputs(rng, S, 5 * 7)
        got, _ = _run_slabs(lib, slab, 5, 7, 9)
        assert np.array_equal(got.reshape(-1), R.slabs(slab)), S


@pytest.mark.parametrize("n", [64, 256])
def test_slabs_square(lib, n):
    rng = np.random.default_rng(11 + n)
    slab = _slab_inputs(rng, 35, n * n)
    got, _ = _run_slabs(lib, slab, n, n, n)
    assert np.array_equal(got.reshape(-1), R.slabs(slab))


@pytest.mark.parametrize("ccols", [1, 5, 256])
def test_slabs_with_colsum(lib, ccols):
    D = _depth(lib, SLABS)
    rng = np.random.default_rng(12 + ccols)
    for S in (D - 1, 2 * D + 3):
        slab, cslab = _slab_inputs(rng, S, 64 * 24), _slab_inputs(rng, S, ccols)
        got, cgot = _run_slabs(lib, slab, 64, 24, 24, cslab)
        assert np.array_equal(got.reshape(-1), R.slabs(slab)), S
        assert np.array_equal(cgot, R.slabs(cslab)), S


def test_slabs_block_size_threshold(lib):
    # up to 16384 outputs the launcher uses 64-thread workgroups, above that 256-thread ones
    D = _depth(lib, SLABS)
    rng = np.random.default_rng(14)
    slab, cslab = _slab_inputs(rng, D + 1, 128 * 128), _slab_inputs(rng, D + 1, 1)
    got, _ = _run_slabs(lib, slab, 128, 128, 128)
    assert np.array_equal(got.reshape(-1), R.slabs(slab))
    got, cgot = _run_slabs(lib, slab, 128, 128, 128, cslab)
    assert np.array_equal(got.reshape(-1), R.slabs(slab)) and np.array_equal(cgot, R.slabs(cslab))


def test_slabs_colsum_only(lib):
    # the library reduces column sums alone as a one-row slab list
    D = _depth(lib, SLABS)
    rng = np.random.default_rng(13)
    for cols in (1, 200, 1024):
        slab = _slab_inputs(rng, 2 * D + 3, cols)
        got, _ = _run_slabs(lib, slab, 1, cols, cols)
        assert np.array_equal(got.reshape(-1), R.slabs(slab)), cols


# ---------------------------------------------------------------- bn_stage1
def _run_bn(lib, a, b, N, tile_rows, P, forward):
    Rr, ld = a.shape
    out = torch.full((R.BN_SLICES, 3, N), -7.0, dtype=torch.float64, device="cuda")
    da, db = _dev(a), _dev(b)
    rc = lib.prh_test_reduce_bn_stage1(_p(da), _p(db), Rr, ld, N, tile_rows, P, forward, _p(out), 0, _st())
    assert rc == 0, lib.prh_last_error()
    torch.cuda.synchronize()
    return out.cpu().numpy()


def _bn_inputs(rng, Rr, N, ld, pair_a, pair_b, across=False):
    a, b = R.gauss(rng, Rr, ld), np.abs(R.gauss(rng, Rr, ld))
    for groups in R.bn_groups(Rr):
        if pair_a:
            R.with_pairs(rng, a[:, :N], groups, R.BIG64, across)
        if pair_b:
            R.with_pairs(rng, b[:, :N], groups, R.BIG64, across)
    return a, b


def _bn_rows(lib):
    # chains of 0-1 terms; of D/2 - 1 and D/2 (the two-stream passes batch D/2 rows); of D and D + 1
    D = _depth(lib, BN1)
    return (1, 31, 33, 8 * (D // 2) * 32 - 3, 8 * D * 32 + 5)


@pytest.mark.parametrize("N,ld", [(32, 36), (40, 44), (64, 72)])
def test_bn_stage1_backward(lib, N, ld):
    rng = np.random.default_rng(20 + N)
    for Rr in _bn_rows(lib):
        for across in (False, True):
            a, b = _bn_inputs(rng, Rr, N, ld, True, True, across)
            got = _run_bn(lib, a, b, N, 64, Rr * 64, 0)
            assert np.array_equal(got, R.bn_stage1(a, b, N, 64, Rr * 64, 0)), (Rr, across)


@pytest.mark.parametrize("N,ld", [(32, 36), (40, 44), (64, 72)])
def test_bn_stage1_forward(lib, N, ld):
    # P: a short last tile (37 rows of 64), and tiles past P (the epilogue's row-tile count can
    # exceed ceil(P / tile_rows)): they count 0 rows and are skipped in the M2 pass
    rng = np.random.default_rng(30 + N)
    for Rr in _bn_rows(lib):
        for P in (Rr * 64, max(1, (Rr - 3) * 64 + 37)):
            for pair_a in (True, False):
                a, b = _bn_inputs(rng, Rr, N, ld, pair_a, not pair_a)
                got = _run_bn(lib, a, b, N, 64, P, 1)
                assert np.array_equal(got, R.bn_stage1(a, b, N, 64, P, 1)), (Rr, P, pair_a)


# ---------------------------------------------------------------- partials_reduce
@pytest.mark.parametrize("N", [40, 64])
def test_partials(lib, N):
    D = _depth(lib, PARTIALS)
    rng = np.random.default_rng(40 + N)
    # chains of 1, 0-1, D-1, D / D+1, 2D / 2D+1 (the one-stream pass batches 2D loads), 2D+3 terms
    for R2 in (1, 31, 32 * (D - 1), 32 * D + 5, 32 * 2 * D + 5, 32 * (2 * D + 3)):
        groups = R.strided_groups(R2, 32)
        for across in (False, True):
            a = R.with_pairs(rng, R.gauss(rng, R2, N), groups, R.BIG64, across)
            b = R.with_pairs(rng, R.gauss(rng, R2, N), groups, R.BIG64, across)
            for use_b, want_a, want_b in ((True, True, True), (False, True, True), (True, False, True), (True, True, False)):
                oa = torch.full((N,), -7.0, device="cuda") if want_a else None
                ob = torch.full((N,), -7.0, device="cuda") if want_b else None
                da, db = _dev(a), _dev(b if use_b else None)
                rc = lib.prh_test_reduce_partials(_p(da), _p(db), R2, N, _p(oa), _p(ob), 0, _st())
                assert rc == 0, lib.prh_last_error()
                torch.cuda.synchronize()
                ra, rb = R.partials(a, b if use_b else None)
                if want_a:
                    assert np.array_equal(oa.cpu().numpy(), ra), (R2, across, use_b)
                if want_b:
                    assert np.array_equal(ob.cpu().numpy(), rb), (R2, across, use_b)


# ---------------------------------------------------------------- ln_param_grad
def test_ln_param_grad(lib):
    D = _depth(lib, LN)
    rng = np.random.default_rng(50)
    for nb in (1, 3, 4 * D + 2, 4 * (2 * D + 3), 512):
        groups = R.strided_groups(nb, 4)
        for across in (False, True):
            g = R.with_pairs(rng, R.gauss(rng, nb, 256), groups, R.BIG64, across)
            b = R.with_pairs(rng, R.gauss(rng, nb, 256), groups, R.BIG64, across)
            og, ob = torch.empty(256, device="cuda"), torch.empty(256, device="cuda")
            dg, db = _dev(g), _dev(b)
            rc = lib.prh_test_reduce_ln_param_grad(_p(dg), _p(db), nb, _p(og), _p(ob), 0, _st())
            assert rc == 0, lib.prh_last_error()
            torch.cuda.synchronize()
            rg, rb = R.ln_param_grad(g, b)
            assert np.array_equal(og.cpu().numpy(), rg) and np.array_equal(ob.cpu().numpy(), rb), (nb, across)


# ---------------------------------------------------------------- the two *_final kernels
def _final_blocks(lib):
    D = _depth(lib, FINAL)
    return (1, 15, 16 * D + 3, 16 * (2 * D + 3))


def test_partial_rows_final(lib):
    rng = np.random.default_rng(60)
    n_el = 3 * 32 + 3                                        # 99: not a multiple of 16
    for nblk in _final_blocks(lib):
        groups = R.strided_groups(nblk, 16)
        for across in (False, True):
            p = R.with_pairs(rng, R.gauss(rng, nblk, n_el), groups, R.BIG32, across)
            ref = R.partial_rows_final(p)
            for n0, want0, want1 in ((96, True, True), (40, True, True), (96, False, True), (96, True, False)):
                o0 = torch.full((n0,), -7.0, device="cuda") if want0 else None
                o1 = torch.full((n_el - n0,), -7.0, device="cuda") if want1 else None
                dp = _dev(p)
                rc = lib.prh_test_reduce_partial_rows_final(_p(dp), nblk, n_el, _p(o0), n0, _p(o1), 0, _st())
                assert rc == 0, lib.prh_last_error()
                torch.cuda.synchronize()
                if want0:
                    assert np.array_equal(o0.cpu().numpy(), ref[:n0]), (nblk, across, n0)
                if want1:
                    assert np.array_equal(o1.cpu().numpy(), ref[n0:]), (nblk, across, n0)


def test_pos_hidden_final(lib):
    rng = np.random.default_rng(61)
    for H in (4, 36, 128):                                   # 4 * H = 16, 144, 512 elements
        for nblk in _final_blocks(lib):
            groups = R.strided_groups(nblk, 16)
            for across in (False, True):
                p = R.with_pairs(rng, R.gauss(rng, nblk, 4 * H), groups, R.BIG32, across)
                dw, db = torch.empty(H, 3, device="cuda"), torch.empty(H, device="cuda")
                dp = _dev(p)
                rc = lib.prh_test_reduce_pos_hidden_final(_p(dp), nblk, H, _p(dw), _p(db), 0, _st())
                assert rc == 0, lib.prh_last_error()
                torch.cuda.synchronize()
                rw, rb = R.pos_hidden_final(p)
                assert np.array_equal(dw.cpu().numpy(), rw) and np.array_equal(db.cpu().numpy(), rb), (H, nblk, across)


# ---------------------------------------------------------------- act_amax
@pytest.mark.parametrize("N,ld", [(40, 44), (64, 64), (2080, 2080)])
def test_act_amax(lib, N, ld):
    # 2080 columns = 65 column blocks: more than the 64 per slice the partial list holds
    rng = np.random.default_rng(70 + N)
    nb = lib.prh_test_reduce_act_amax_workspace_bytes()
    ws = torch.empty(nb, dtype=torch.uint8, device="cuda")
    for Rr in (1, 33, 2049):
        z = R.gauss(rng, Rr, ld)
        c, d = z + np.abs(R.gauss(rng, Rr, ld)), z
        scale, shift = R.gauss(rng, N), R.gauss(rng, N)
        out = torch.full((1,), -7.0, device="cuda")
        dc, dd, dsc, dsh = _dev(c), _dev(d), _dev(scale), _dev(shift)
        rc = lib.prh_test_reduce_act_amax(_p(dc), _p(dd), Rr, ld, N, _p(dsc), _p(dsh), _p(out), _p(ws), nb, 0, _st())
        assert rc == 0, lib.prh_last_error()
        torch.cuda.synchronize()
        assert out.cpu().numpy()[0] == R.act_amax(c, d, N, scale, shift), Rr
