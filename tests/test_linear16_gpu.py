"""The wide K / V projections of the bf16 mode at the C ABI: prh_linear_forward_out16 (fp32 x -> bf16 y) and
prh_linear_backward_dy16 (bf16 dy -> fp32 dx, dw, db), which only whole-model tests reached.  As for the encoder
Linears in tests/test_bf16_gpu.py the reference is fp64 arithmetic on the SAME rounded operands (bf16(x), bf16(w), the
bf16 dy as given), so what is left is fp32 accumulation - and, for y, its one rounding to bf16.

Shapes: the decoder's own k = 256 / n = 6 * 256 at one row, one row past a 256-row tile and an odd 4099; n off the
256-column tile; K % 64 == 0 (DMA core for the bf16-input dgrad) and K = 8 / 72 (register-staged core)."""
import ctypes as C

import pytest
import torch

pytestmark = pytest.mark.gpu

SHAPES = [(1, 256, 1536), (257, 256, 1536), (4099, 256, 1536), (515, 64, 72), (300, 8, 8), (777, 72, 128)]
PAD = 5                  # sentinel rows behind y
NAN16 = 0x7FC0


def _p(t):
    return C.c_void_p(0 if t is None else t.data_ptr())


def _bf(t):
    return t.to(torch.bfloat16)


@pytest.fixture()
def bf16_mode():
    from pointnet_refine_amd import _lib
    lib = _lib.lib()
    old = lib.prh_get_gemm_mode()
    assert lib.prh_set_gemm_mode(4) == 0
    yield lib
    lib.prh_set_gemm_mode(old)


def _operands(rows, k, n):
    g = torch.Generator().manual_seed(rows + k + n)
    x = torch.randn(rows, k, generator=g).cuda()
    w = (torch.randn(n, k, generator=g) / k ** 0.5).cuda()
    b = torch.randn(n, generator=g).cuda()
    dy = _bf(torch.randn(rows, n, generator=g)).cuda()
    return x, w, b, dy


def _workspace(lib, rows, k, n, backward):
    nb = lib.prh_linear_bf16_workspace_bytes(rows, k, n, backward)
    return torch.empty(nb, dtype=torch.uint8, device="cuda"), nb


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _nan(*shape):
    return torch.full(shape, float("nan"), device="cuda")


def _check_dx(dx, dy, w):
    ref = dy.double() @ _bf(w).double()
    assert float((dx.double() - ref).norm() / ref.norm()) < 2e-6
    assert float((dx.double() - ref).abs().max()) < 1e-4 * float(ref.abs().max())


def _check_dw_db(dw, db, dy, x):
    if dw is not None:
        ref = dy.double().t() @ _bf(x).double()
        assert float((dw.double() - ref).norm() / ref.norm()) < 2e-6
    if db is not None:
        rdb = dy.double().sum(0)
        assert float((db.double() - rdb).abs().max()) < 1e-4 * float(rdb.abs().max()) + 1e-4


@pytest.mark.parametrize("rows,k,n", SHAPES)
def test_out16_forward_is_exact_on_rounded_operands(bf16_mode, rows, k, n):
    """y (bf16) against fp64 on bf16(x), bf16(w), b: one rounding to bf16 (2^-8 of the value) on top of the fp32 gate
    of the fp32-output kernel, elementwise; the rows behind the last one keep their sentinel bits.  Largest error / bound
    on an MI355X: 0.90 to 0.95 over the six shapes - the rounding itself (2^-8 of a value just above a power of two)."""
    lib = bf16_mode
    x, w, b, _ = _operands(rows, k, n)
    ws, nb = _workspace(lib, rows, k, n, 0)
    y = torch.full((rows + PAD, n), NAN16, dtype=torch.int16, device="cuda").view(torch.bfloat16)
    assert lib.prh_linear_forward_out16(_p(x), k, _p(w), _p(b), _p(y), rows, k, n, _p(ws), nb, 0, _stream()) == 0
    ref = _bf(x).double() @ _bf(w).double().t() + b.double()
    err = (y[:rows].double() - ref).abs()
    bound = 2.0 ** -8 * ref.abs() + 1e-4 * float(ref.abs().max())
    print(f"out16 ({rows}, {k}, {n}): largest error / bound {float((err / bound).max()):.3f}")
    assert bool((err <= bound).all())                                 # a NaN left in y fails this, too
    assert bool((y[rows:].view(torch.int16) == NAN16).all())
    # the fp32 bias alone, without the product: the epilogue's column indexing
    y0 = torch.full((rows + PAD, n), NAN16, dtype=torch.int16, device="cuda").view(torch.bfloat16)
    assert lib.prh_linear_forward_out16(_p(torch.zeros_like(x)), k, _p(w), _p(b), _p(y0), rows, k, n, _p(ws), nb, 0,
                                        _stream()) == 0
    assert torch.equal(y0[:rows], _bf(b).expand(rows, n))


@pytest.mark.parametrize("rows,k,n", SHAPES)
def test_dy16_backward_is_exact_on_rounded_operands(bf16_mode, rows, k, n):
    """dx = dy bf16(w), dw = dy^T bf16(x), db = column sums of dy - all three outputs fp32, the gates those of
    test_linear_bf16_kernels_are_exact_on_rounded_operands for fp32 outputs; then with dx, and with dw and db, left out."""
    lib = bf16_mode
    x, w, _, dy = _operands(rows, k, n)
    ws, nb = _workspace(lib, rows, k, n, 1)
    bwd = lib.prh_linear_backward_dy16
    dx, dw, db = _nan(rows, k), _nan(n, k), _nan(n)
    assert bwd(_p(x), k, _p(w), _p(dy), _p(dx), _p(dw), _p(db), rows, k, n, _p(ws), nb, 0, _stream()) == 0
    _check_dx(dx, dy, w)
    _check_dw_db(dw, db, dy, x)
    dw2, db2 = _nan(n, k), _nan(n)
    assert bwd(_p(x), k, _p(w), _p(dy), None, _p(dw2), _p(db2), rows, k, n, _p(ws), nb, 0, _stream()) == 0
    _check_dw_db(dw2, db2, dy, x)
    dx2 = _nan(rows, k)
    assert bwd(_p(x), k, _p(w), _p(dy), _p(dx2), None, None, rows, k, n, _p(ws), nb, 0, _stream()) == 0
    _check_dx(dx2, dy, w)


def test_out16_dy16_read_x_through_its_leading_dimension(bf16_mode):
    """x as the first k columns of wider rows (ldx > k), NaN behind them."""
    lib = bf16_mode
    rows, k, n, ldx = 515, 64, 72, 68
    x, w, b, dy = _operands(rows, k, n)
    xw = _nan(rows, ldx)
    xw[:, :k] = x
    ws, nb = _workspace(lib, rows, k, n, 1)
    y = torch.full((rows, n), NAN16, dtype=torch.int16, device="cuda").view(torch.bfloat16)
    assert lib.prh_linear_forward_out16(_p(xw), ldx, _p(w), _p(b), _p(y), rows, k, n, _p(ws), nb, 0, _stream()) == 0
    ref = _bf(x).double() @ _bf(w).double().t() + b.double()
    assert bool(((y.double() - ref).abs() <= 2.0 ** -8 * ref.abs() + 1e-4 * float(ref.abs().max())).all())
    dw, db = _nan(n, k), _nan(n)
    assert lib.prh_linear_backward_dy16(_p(xw), ldx, _p(w), _p(dy), None, _p(dw), _p(db), rows, k, n, _p(ws), nb, 0,
                                        _stream()) == 0
    _check_dw_db(dw, db, dy, x)


def test_out16_dy16_refuse_bad_arguments(bf16_mode):
    """k % 8 != 0 is refused by the backward; a workspace one byte shorter than prh_linear_bf16_workspace_bytes reports
    is refused by both.  Nothing is written."""
    lib = bf16_mode
    rows, n = 64, 16
    for k, short in ((12, 0), (16, 1)):
        x, w, b, dy = _operands(rows, k, n)
        ws, nb = _workspace(lib, rows, k, n, 1)
        nb0 = lib.prh_linear_bf16_workspace_bytes(rows, k, n, 0)
        dx, dw, db = _nan(rows, k), _nan(n, k), _nan(n)
        y = torch.full((rows, n), NAN16, dtype=torch.int16, device="cuda").view(torch.bfloat16)
        assert lib.prh_linear_backward_dy16(_p(x), k, _p(w), _p(dy), _p(dx), _p(dw), _p(db), rows, k, n, _p(ws), nb - short,
                                            0, _stream()) != 0
        assert lib.prh_last_error()
        if short:
            assert lib.prh_linear_forward_out16(_p(x), k, _p(w), _p(b), _p(y), rows, k, n, _p(ws), nb0 - short, 0,
                                                _stream()) != 0
        torch.cuda.synchronize()
        assert bool(torch.isnan(dx).all() and torch.isnan(dw).all() and torch.isnan(db).all())
        assert bool((y.view(torch.int16) == NAN16).all())
        if short:       # and the reported sizes are enough
            assert lib.prh_linear_backward_dy16(_p(x), k, _p(w), _p(dy), _p(dx), _p(dw), _p(db), rows, k, n, _p(ws), nb, 0,
                                                _stream()) == 0
            assert lib.prh_linear_forward_out16(_p(x), k, _p(w), _p(b), _p(y), rows, k, n, _p(ws), nb0, 0, _stream()) == 0
            _check_dx(dx, dy, w)
            _check_dw_db(dw, db, dy, x)


def test_bf16_input_linear_refuses_a_short_workspace(bf16_mode):
    """The same rule for the two entries that share the workspace layout (prh_linear_forward_bf16 / _backward_bf16)."""
    lib = bf16_mode
    rows, k, n = 64, 16, 16
    x, w, b, dy = _operands(rows, k, n)
    x16, dyf = _bf(x), dy.float()
    ws, nb = _workspace(lib, rows, k, n, 1)
    nb0 = lib.prh_linear_bf16_workspace_bytes(rows, k, n, 0)
    y, dw, db = _nan(rows, n), _nan(n, k), _nan(n)
    dx = torch.full((rows, k), NAN16, dtype=torch.int16, device="cuda").view(torch.bfloat16)
    assert lib.prh_linear_forward_bf16(_p(x16), k, _p(w), _p(b), _p(y), rows, k, n, 0, _p(ws), nb0 - 1, 0, _stream()) != 0
    assert lib.prh_linear_backward_bf16(_p(x16), k, _p(w), _p(dyf), _p(dx), _p(dw), _p(db), rows, k, n, _p(ws), nb - 1, 0,
                                        _stream()) != 0
    torch.cuda.synchronize()
    assert bool(torch.isnan(y).all() and torch.isnan(dw).all() and torch.isnan(db).all())
    assert bool((dx.view(torch.int16) == NAN16).all())
    assert lib.prh_linear_forward_bf16(_p(x16), k, _p(w), _p(b), _p(y), rows, k, n, 0, _p(ws), nb0, 0, _stream()) == 0
    ref = x16.double() @ _bf(w).double().t() + b.double()
    assert float((y.double() - ref).norm() / ref.norm()) < 2e-6
