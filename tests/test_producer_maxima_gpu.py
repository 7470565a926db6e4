"""Operand maxima taken where the operand is written, and the gradient fan-in at `memory` summed in a dgrad epilogue.

A split-fp16 GEMM (GEMM mode 3) places each operand by a power-of-two scale from the operand's largest magnitude.
Where a kernel of ours has just written that operand, it reports the maximum itself (prh_linear_forward_amax,
prh_linear_backward_amax, prh_pos_hidden_forward_amax) instead of a read pass (prh_operand_absmax).  A maximum
does not depend on the order of reduction, so every comparison here is == on the fp32 value, and everything
computed with a produced maximum must equal, bit for bit, what the measured maximum gives.
"""
import copy
import ctypes as C

import pytest
import torch

from oracle import procedural as P

pytestmark = pytest.mark.gpu

# rows, k, n: second-generation core with ragged rows and a partial last column tile (n % 256 != 0); the K / V
# projection shape; below the grid floor of the split cores (fallback: the output is measured after the GEMM)
SHAPES = [(8229, 64, 260), (8192, 256, 1536), (700, 256, 256)]
# ... plus, for the backward, a dgrad that lands on the second-generation core with ragged rows (N = k = 256, K = n = 512)
BWD_SHAPES = SHAPES + [(8229, 256, 512)]


def _p(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def _st():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _dev():
    return torch.cuda.current_device()


@pytest.fixture()
def lib():
    from pointnet_refine_amd import _lib
    l = _lib.lib()
    old = l.prh_get_gemm_mode()
    assert l.prh_set_gemm_mode(3) == 0
    yield l
    l.prh_set_gemm_mode(old)


def _operands(rows, k, n, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(rows, k, generator=g).cuda()
    w = (torch.randn(n, k, generator=g) / k ** 0.5).cuda()
    b = torch.randn(n, generator=g).cuda()
    r = torch.randn(rows, n, generator=g).cuda()
    return x, w, b, r


def _fwd(lib, x, w, b, resid=None, relu=0, p=0.0, seed=0, xa=None, amax=True, full=False):
    """(y, max|y| reported) through prh_linear_forward_amax; full: through prh_linear_forward_full."""
    rows, k = x.shape
    n = w.shape[0]
    nb = lib.prh_linear_forward_workspace_bytes(rows, k, n)
    ws = torch.empty(nb, dtype=torch.uint8, device="cuda")
    y = torch.full((rows, n), float("nan"), device="cuda")
    out = torch.full((1,), float("nan"), device="cuda") if amax else None
    if full:
        rc = lib.prh_linear_forward_full(_p(x), k, _p(w), _p(b), _p(resid), n, _p(y), rows, k, n, relu, _p(xa), None,
                                         C.c_float(p), seed, _p(ws), nb, _dev(), _st())
    else:
        rc = lib.prh_linear_forward_amax(_p(x), k, _p(w), _p(b), _p(resid), n, _p(y), rows, k, n, relu, _p(xa), None,
                                         C.c_float(p), seed, _p(out), _p(ws), nb, _dev(), _st())
    assert rc == 0, lib.prh_last_error()
    return y, out


def _bwd(lib, x, w, dy, dx=None, acc=0, amax=False, xa=None, da=None, full=False):
    """(dx, dw, db, max|dx| reported); dx given: the buffer the call writes (the addend when acc)."""
    rows, k = x.shape
    n = w.shape[0]
    nb = lib.prh_linear_backward_workspace_bytes(rows, k, n)
    ws = torch.empty(nb, dtype=torch.uint8, device="cuda")
    if dx is None:
        dx = torch.full((rows, k), float("nan"), device="cuda")
    dw = torch.full((n, k), float("nan"), device="cuda")
    db = torch.full((n,), float("nan"), device="cuda")
    out = torch.full((1,), float("nan"), device="cuda") if amax else None
    if full:
        rc = lib.prh_linear_backward_full(_p(x), k, _p(w), _p(dy), _p(dx), _p(dw), _p(db), rows, k, n, _p(xa), _p(da),
                                          None, _p(ws), nb, _dev(), _st())
    else:
        rc = lib.prh_linear_backward_amax(_p(x), k, _p(w), _p(dy), _p(dx), _p(dw), _p(db), rows, k, n, _p(xa), _p(da),
                                          None, acc, _p(out), _p(ws), nb, _dev(), _st())
    assert rc == 0, lib.prh_last_error()
    return dx, dw, db, out


# ------------------------------------------------------------------------------------------
# C ABI, mode 3
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rows,k,n", SHAPES)
def test_forward_maximum_equals_the_outputs_maximum(lib, rows, k, n):
    """plain, ReLU, residual, ReLU + dropout(0.1): the reported value == y.abs().max(), and y has the bits of
    prh_linear_forward_full (the output pointer changes nothing else)."""
    x, w, b, r = _operands(rows, k, n, seed=rows + n)
    for name, kw in (("plain", {}), ("relu", dict(relu=1)), ("resid", dict(resid=r)),
                     ("relu+dropout", dict(relu=1, p=0.1, seed=1234))):
        y, a = _fwd(lib, x, w, b, **kw)
        y0, _ = _fwd(lib, x, w, b, full=True, amax=False, **kw)
        ynull, _ = _fwd(lib, x, w, b, amax=False, **kw)
        assert bool(torch.isfinite(y).all()), name
        assert float(a) == float(y.abs().max()), (name, float(a), float(y.abs().max()))
        assert torch.equal(y, y0) and torch.equal(ynull, y0), name
        if name == "relu+dropout":
            assert float((y == 0).float().mean()) > 0.52      # half by the ReLU, a tenth of the rest dropped


def test_forward_maximum_ignores_rows_and_columns_outside_the_matrix(lib):
    """Columns 3 and n - 1: bias +-100, and the rows of x cancel it exactly (x[:, 0] = 1, w[c, 0] = -+100, the
    rest of w[c] zero), so every stored output there is 0 while a padded row (x = 0) would give |b| = 100."""
    rows, k, n = 8229, 64, 260
    x, w, b, _ = _operands(rows, k, n, seed=3)
    x[:, 0] = 1.0
    for c, s in ((3, 1.0), (n - 1, -1.0)):
        w[c] = 0.0
        w[c, 0] = -100.0 * s
        b[c] = 100.0 * s
    y, a = _fwd(lib, x, w, b)
    assert float(y[:, 3].abs().max()) == 0.0 and float(y[:, n - 1].abs().max()) == 0.0
    assert float(a) == float(y.abs().max()) and float(a) < 50.0, float(a)


@pytest.mark.parametrize("rows,k,n", SHAPES)
def test_forward_maximum_finds_a_planted_element_anywhere(lib, rows, k, n):
    x, w, b, r = _operands(rows, k, n, seed=11)
    g = torch.Generator().manual_seed(rows)
    rnd = (int(torch.randint(0, rows, (1,), generator=g)), int(torch.randint(0, n, (1,), generator=g)))
    for (i, j), v in (((0, 0), 1000.0), ((rows - 1, n - 1), -1000.0), (rnd, -1000.0)):
        rr = r.clone()
        rr[i, j] = v
        y, a = _fwd(lib, x, w, b, resid=rr)
        assert int(y.abs().argmax()) == i * n + j
        assert float(a) == float(y.abs().max()) == abs(float(y[i, j]))


@pytest.mark.parametrize("rows,k,n", SHAPES)
def test_forward_maximum_drops_a_nan(lib, rows, k, n):
    """fmaxf semantics, as the stand-alone pass (test_operand_absmax_edge_values_and_errors): a NaN output is
    dropped, the maximum of the finite outputs is reported."""
    x, w, b, r = _operands(rows, k, n, seed=5)
    r[rows // 2, n // 3] = float("nan")
    r[rows - 1, 0] = float("nan")
    y, a = _fwd(lib, x, w, b, resid=r)
    assert int(torch.isnan(y).sum()) == 2
    assert float(a) == float(y[~torch.isnan(y)].abs().max())


@pytest.mark.parametrize("rows,k,n", BWD_SHAPES)
def test_backward_accumulates_into_dx_and_reports_its_maximum(lib, rows, k, n):
    """dx_accumulate: dx == addend + dx_plain bit for bit (one fp32 addition per element whichever kernel makes
    it); dx_amax_out == max|dx| with and without the addend; dw, db and a NULL pointer change nothing."""
    x, w, _, _ = _operands(rows, k, n, seed=rows + k)
    g = torch.Generator().manual_seed(n)
    dy = torch.randn(rows, n, generator=g).cuda()
    addend = (torch.randn(rows, k, generator=g) * 3).cuda()
    dx0, dw0, db0, _ = _bwd(lib, x, w, dy, full=True)
    dx1, dw1, db1, a1 = _bwd(lib, x, w, dy, amax=True)
    assert torch.equal(dx1, dx0) and torch.equal(dw1, dw0) and torch.equal(db1, db0)
    assert float(a1) == float(dx0.abs().max())
    dxn, _, _, _ = _bwd(lib, x, w, dy)
    assert torch.equal(dxn, dx0)
    want = addend + dx0
    dx2, dw2, db2, a2 = _bwd(lib, x, w, dy, dx=addend.clone(), acc=1, amax=True)
    assert torch.equal(dx2, want)
    assert float(a2) == float(want.abs().max())
    assert torch.equal(dw2, dw0) and torch.equal(db2, db0)
    dx3, _, _, _ = _bwd(lib, x, w, dy, dx=addend.clone(), acc=1)
    assert torch.equal(dx3, want)


@pytest.mark.parametrize("rows", [8229, 5])
def test_pos_hidden_maximum(lib, rows):
    g = torch.Generator().manual_seed(rows)
    ctx = (torch.randn(rows, 4, generator=g) * 20).cuda()      # points read in place from 4-wide rows
    w0 = torch.randn(256, 3, generator=g).cuda()
    b0 = torch.randn(256, generator=g).cuda()
    h0 = torch.full((rows, 256), float("nan"), device="cuda")
    assert lib.prh_pos_hidden_forward(_p(ctx), 4, _p(w0), _p(b0), _p(h0), rows, 256, _dev(), _st()) == 0
    nb = lib.prh_pos_hidden_forward_workspace_bytes()
    ws = torch.empty(nb, dtype=torch.uint8, device="cuda")
    for want in (True, False):
        h = torch.full((rows, 256), float("nan"), device="cuda")
        a = torch.full((1,), float("nan"), device="cuda") if want else None
        assert lib.prh_pos_hidden_forward_amax(_p(ctx), 4, _p(w0), _p(b0), _p(h), rows, 256, _p(a), _p(ws), nb,
                                               _dev(), _st()) == 0, lib.prh_last_error()
        assert torch.equal(h, h0)
        if want:
            assert float(a) == float(h0.max()) > 0.0


def test_supplied_produced_maxima_equal_measured_ones(lib):
    """Two chained Linears of 8192 rows, 256 -> 256 -> 256 (both on the split-fp16 cores): the second one's forward
    with x_amax = the first one's reported output maximum, and the first one's backward with dy_amax = the
    second one's reported dx maximum, against NULL (the launch measures): y, dx, dw, db bit-equal."""
    rows, k = 8192, 256
    assert lib.prh_linear_uses_operand_maxima(rows, k, k) == 1
    x, w1, b1, r = _operands(rows, k, k, seed=21)
    _, w2, b2, _ = _operands(rows, k, k, seed=22)
    g = torch.Generator().manual_seed(23)
    dy = torch.randn(rows, k, generator=g).cuda()
    h, ha = _fwd(lib, x, w1, b1, resid=r)
    y_s, _ = _fwd(lib, h, w2, b2, xa=ha, amax=False)
    y_m, _ = _fwd(lib, h, w2, b2, amax=False)
    assert torch.equal(y_s, y_m)
    dh_s, dw2_s, db2_s, da = _bwd(lib, h, w2, dy, amax=True, xa=ha)
    dh_m, dw2_m, db2_m, _ = _bwd(lib, h, w2, dy)
    assert torch.equal(dh_s, dh_m) and torch.equal(dw2_s, dw2_m) and torch.equal(db2_s, db2_m)
    dx_s, dw1_s, db1_s, _ = _bwd(lib, x, w1, dh_s, da=da)
    dx_m, dw1_m, db1_m, _ = _bwd(lib, x, w1, dh_s)
    assert torch.equal(dx_s, dx_m) and torch.equal(dw1_s, dw1_m) and torch.equal(db1_s, db1_m)


# ------------------------------------------------------------------------------------------
# Model: ops.PRODUCER_MAXIMA on against off
# ------------------------------------------------------------------------------------------
def _train_step(B, N, M, chunk, on, census=None, profile=False):
    """One seeded TrainStep.forward_backward of LineRefineNet -> (flat gradients, out, profiler or None)."""
    from pointnet_refine_amd import ops
    from pointnet_refine_amd.model import LineRefineNet
    from pointnet_refine_amd.train_step import TrainStep
    m = LineRefineNet()
    m.load_state_dict(P.linerefine_state_dict(0), strict=True)
    m = m.cuda().train()
    ctx, noisy, target = P.synth_batch(B, N, 4, M, seed=7)
    ctx, noisy, target = ctx.cuda(), noisy.cuda(), target.cuda()
    st = TrainStep(m, None, decoder_chunk=chunk)
    st.keep_out = True
    old, ops.PRODUCER_MAXIMA = ops.PRODUCER_MAXIMA, on
    real = ops.operand_absmax
    if census is not None:
        def counted(t):
            census.append(tuple(t.shape))
            return real(t)
        ops.operand_absmax = counted
    prof = None
    try:
        torch.manual_seed(123)              # the dropout seeds are drawn from the default generator
        st.grads.zero()
        if profile:
            from torch.profiler import ProfilerActivity, profile as tprofile
            with tprofile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA], record_shapes=True) as prof:
                st.forward_backward(ctx, noisy, target)
                torch.cuda.synchronize()
        else:
            st.forward_backward(ctx, noisy, target)
        torch.cuda.synchronize()
        return st.grads.flat.detach().clone(), st.last_out.clone(), prof, copy.copy(st.grads.offsets), m
    finally:
        ops.PRODUCER_MAXIMA = old
        ops.operand_absmax = real
        st.close()


@pytest.mark.parametrize("B,N,M,chunk", [(16, 512, 32, None), (5, 300, 7, None), (16, 512, 32, 8)],
                         ids=["split-cores", "every-fallback", "decoder-chunk-8"])
def test_model_step_is_bit_identical_with_producer_maxima(lib, B, N, M, chunk):
    g_on, out_on, _, offs, m = _train_step(B, N, M, chunk, True)
    g_off, out_off, _, _, _ = _train_step(B, N, M, chunk, False)
    assert bool(torch.isfinite(g_on).all()) and float(g_on.abs().max()) > 0.0
    assert torch.equal(out_on, out_off)
    names = [n for n, p in m.named_parameters() if p.requires_grad]
    bad = [n for n, o, p in zip(names, offs, [p for p in m.parameters() if p.requires_grad])
           if not torch.equal(g_on[o:o + p.numel()], g_off[o:o + p.numel()])]
    assert not bad, bad
    assert torch.equal(g_on, g_off)


def test_no_read_pass_and_no_stock_add_over_the_context_rows(lib):
    """During a step with the switch on, ops.operand_absmax is never called on a (B*N)-row tensor (h, mempos,
    memory, d_mempos and d_memory arrive with their maxima), and no aten::add takes a (B, N, 256) input (the
    fan-in at `memory` is summed in the V projection's dgrad epilogue).  With the switch off both exist."""
    B, N, M = 16, 512, 32
    for on in (True, False):
        census = []
        _, _, prof, _, _ = _train_step(B, N, M, None, on, census=census, profile=True)
        wide = [s for s in census if s[0] == B * N]
        adds = [e for e in prof.events() if e.name in ("aten::add", "aten::add_")
                and any(list(s) == [B, N, 256] for s in (e.input_shapes or []) if isinstance(s, (list, tuple)))]
        print(f"PRODUCER_MAXIMA={on}: operand_absmax on {B * N} rows: {wide}; aten::add over (B, N, 256): {len(adds)}")
        if on:
            assert wide == [] and adds == []
        else:
            assert len(wide) >= 3 and len(adds) >= 1
