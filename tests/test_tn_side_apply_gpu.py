"""The BatchNorm-backward apply pass carried inside the transposed-read wgrad launch
(gemm_tn_tr_kernel<PROB, SIDE = true>) against the stand-alone pass and the plain wgrad, bit for bit,
through the raw-core export prh_test_gemm_tn_side."""
import ctypes as C

import pytest
import torch

pytestmark = pytest.mark.gpu

MO, NI, LD = 128, 64, 448          # wgrad widths; leading dimension of the side matrices (> cols)
PAD = -123.0                       # what the pad columns hold before the pass


def _p(t):
    return C.c_void_p(t.data_ptr())


@pytest.fixture(scope="module")
def lib():
    from pointnet_refine_amd import _lib
    l = _lib.lib()
    old = l.prh_get_gemm_mode()
    assert l.prh_set_gemm_mode(3) == 0      # split-fp16 cores: the only mode with the side job
    yield l
    l.prh_set_gemm_mode(old)


def _operands(p):
    g = torch.Generator(device="cuda").manual_seed(p)
    a = torch.randn(p, MO, device="cuda", generator=g)
    b = torch.randn(p, NI, device="cuda", generator=g)
    return a, b


def _side(rows, cols, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    dy = torch.full((rows, LD), PAD, device="cuda")
    z = torch.full((rows, LD), PAD, device="cuda")
    dy[:, :cols] = torch.randn(rows, cols, device="cuda", generator=g)
    z[:, :cols] = torch.randn(rows, cols, device="cuda", generator=g) * 3 + 1
    ka, kb, kc = (torch.randn(cols, device="cuda", generator=g) for _ in range(3))
    return dy, z, ka, kb, kc


def _run(lib, a, b, dy, z, ka, kb, kc, rows, cols, side):
    p = a.shape[0]
    c = torch.full((MO, NI), float("nan"), device="cuda")
    cs = torch.full((MO,), float("nan"), device="cuda")
    amax = torch.full((1,), float("nan"), device="cuda")
    nb = lib.prh_test_gemm_tn_side_workspace_bytes(p, MO, NI)
    ws = torch.empty(nb, dtype=torch.uint8, device="cuda")
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    rc = lib.prh_test_gemm_tn_side(_p(a), _p(b), _p(c), _p(cs), p, MO, NI, _p(dy), LD, _p(z), LD, _p(ka), _p(kb),
                                   _p(kc), rows, cols, side, _p(amax), _p(ws), nb, 0, st)
    assert rc == 0, lib.prh_last_error()
    torch.cuda.synchronize()
    return c, cs, amax


def _plain(lib, a, b):
    p = a.shape[0]
    c = torch.full((MO, NI), float("nan"), device="cuda")
    cs = torch.full((MO,), float("nan"), device="cuda")
    nb = lib.prh_test_gemm_tn_workspace_bytes(p, MO, NI)
    ws = torch.empty(nb, dtype=torch.uint8, device="cuda")
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    assert lib.prh_test_gemm_tn(_p(a), _p(b), _p(c), _p(cs), p, MO, NI, _p(ws), nb, 0, st) == 0, lib.prh_last_error()
    torch.cuda.synchronize()
    return c, cs


def _check(lib, p, rows, cols):
    a, b = _operands(p)
    dy0, z, ka, kb, kc = _side(rows, cols, p + cols)
    c_ref, cs_ref = _plain(lib, a, b)
    dy_alone = dy0.clone()
    _, _, amax_alone = _run(lib, a, b, dy_alone, z, ka, kb, kc, rows, cols, 0)
    dy_side = dy0.clone()
    c, cs, amax = _run(lib, a, b, dy_side, z, ka, kb, kc, rows, cols, 1)
    # (a) the carrier computes what the plain launch computes
    assert torch.equal(c, c_ref) and torch.equal(cs, cs_ref)
    # (b) every element as the stand-alone pass writes it (and that pass did something)
    assert torch.equal(dy_side, dy_alone)
    assert not torch.equal(dy_alone[:, :cols], dy0[:, :cols])
    # (c) the reduced maximum is the maximum of what was written, and the stand-alone pass's
    assert float(amax) == float(dy_side[:, :cols].abs().max()) == float(amax_alone)
    # (d) pad columns untouched
    assert bool((dy_side[:, cols:] == PAD).all())


@pytest.mark.parametrize("cols", [64, 68])
@pytest.mark.parametrize("p", [8192, 9995])
def test_side_apply_matches_stand_alone_and_plain_wgrad(lib, p, cols):
    _check(lib, p, p, cols)


@pytest.mark.parametrize("cols", [64, 68])
def test_side_apply_with_fewer_rows_than_slices(lib, cols):
    """(e) rows = 5: fewer rows than the grid has wave slices; every element is still written."""
    _check(lib, 8192, 5, cols)


def test_side_apply_walks_column_chunks(lib):
    """cols = 324 > 256: a wave walks its row in 256-column chunks, the last one 68 wide."""
    _check(lib, 9995, 9995, 324)
