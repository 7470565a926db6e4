"""The period of the side walk in the transposed-read wgrad carrier (gemm_tn_tr_kernel<PROB, SIDE = true, Q>):
one item of the carried BatchNorm-backward apply pass per thread every Q = 1, 2 or 4 k-tiles, planned per
launch (tn_side_period) or forced, through the raw-core export prh_test_gemm_tn_side_ex.

The period moves work in time and nothing else, so every case asks for the same bits: C and the column
sums of the plain wgrad launch (with BN+ReLU coefficients on B: of the plain <1, false> launch), dy of the
stand-alone apply pass, its maximum, and sentinels in every pad column and every row beyond `rows`.

MO x NI = 128 x 64 is one tile; the plan gives P = 8192 16 splits of 32 k-tiles (128 waves), P = 9995
20 splits whose last has 17 k-tiles (odd, no multiple of 4), P = 19969 40 splits whose last has one row.
"""
import ctypes as C

import pytest
import torch

pytestmark = pytest.mark.gpu

MO, NI, LD = 128, 64, 448          # wgrad widths; leading dimension of the side matrices (> cols)
PAD = -123.0                       # what pad columns and the rows beyond `rows` hold before the pass
EXTRA = 3                          # rows allocated beyond `rows`

# (P, rows, cols) -> planned period
PLANNED = {
    (8192, 2048, 64): 4,           # 512 groups of 4 rows over 128 waves: 4 items per wave, 32 k-tiles
    (8192, 8192, 64): 2,           # 16 items per wave: 2 x 16 = 32 k-tiles, 4 x 16 does not fit
    (9995, 9995, 324): 1,          # two chunks per row: 19990 items for 160 waves x 32 k-tiles; drains
}
# more shapes for the forced periods: a last split of 17 k-tiles, a ragged last column quad, and
# fewer rows than the grid has wave slices (most waves have no item at all)
FORCED_ONLY = [(9995, 9995, 64), (8192, 8192, 68), (8192, 5, 64)]


def _p(t):
    return C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p(0)


@pytest.fixture(scope="module")
def lib():
    from pointnet_refine_amd import _lib
    l = _lib.lib()
    old = l.prh_get_gemm_mode()
    assert l.prh_set_gemm_mode(3) == 0      # split-fp16 cores: the only mode with the side job
    yield l
    l.prh_set_gemm_mode(old)


def _run(lib, a, b, qa, qb, dy, z, ka, kb, kc, rows, cols, side, period):
    p = a.shape[0]
    c = torch.full((MO, NI), float("nan"), device="cuda")
    cs = torch.full((MO,), float("nan"), device="cuda")
    amax = torch.full((1,), float("nan"), device="cuda")
    nb = lib.prh_test_gemm_tn_side_workspace_bytes(p, MO, NI)
    ws = torch.empty(nb, dtype=torch.uint8, device="cuda")
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    used = C.c_int(-1)
    rc = lib.prh_test_gemm_tn_side_ex(_p(a), _p(b), _p(c), _p(cs), p, MO, NI, _p(qa), _p(qb), _p(dy), LD, _p(z), LD,
                                      _p(ka), _p(kb), _p(kc), rows, cols, side, period, C.byref(used), _p(amax),
                                      _p(ws), nb, 0, st)
    assert rc == 0, lib.prh_last_error()
    torch.cuda.synchronize()
    return c, cs, amax, used.value


_REF = {}


def _reference(lib, p, rows, cols, bn):
    """Inputs of one shape and what the stand-alone pass and the plain launch make of them: computed once,
    shared by every period, never written again (each case works on a clone of dy0)."""
    key = (p, rows, cols, bn)
    if key not in _REF:
        g = torch.Generator(device="cuda").manual_seed(p + 7 * rows + cols)
        a = torch.randn(p, MO, device="cuda", generator=g)
        b = torch.randn(p, NI, device="cuda", generator=g)
        qa = qb = None
        if bn:
            qa = torch.rand(NI, device="cuda", generator=g) * 0.5 + 0.75
            qb = torch.randn(NI, device="cuda", generator=g) * 0.3
        dy0 = torch.full((rows + EXTRA, LD), PAD, device="cuda")
        z = torch.full((rows + EXTRA, LD), PAD, device="cuda")
        dy0[:rows, :cols] = torch.randn(rows, cols, device="cuda", generator=g)
        z[:rows, :cols] = torch.randn(rows, cols, device="cuda", generator=g) * 3 + 1
        ka, kb, kc = (torch.randn(cols, device="cuda", generator=g) for _ in range(3))
        dy_alone = dy0.clone()
        c_ref, cs_ref, amax_alone, used = _run(lib, a, b, qa, qb, dy_alone, z, ka, kb, kc, rows, cols, 0, 0)
        assert used == 0                                             # nothing carried
        assert not torch.equal(dy_alone[:rows, :cols], dy0[:rows, :cols])      # the pass did something
        _REF[key] = (a, b, qa, qb, dy0, z, ka, kb, kc, c_ref, cs_ref, dy_alone, float(amax_alone))
    return _REF[key]


def _check(lib, p, rows, cols, period, bn=False):
    a, b, qa, qb, dy0, z, ka, kb, kc, c_ref, cs_ref, dy_alone, amax_alone = _reference(lib, p, rows, cols, bn)
    dy = dy0.clone()
    c, cs, amax, used = _run(lib, a, b, qa, qb, dy, z, ka, kb, kc, rows, cols, 1, period)
    assert torch.equal(c, c_ref) and torch.equal(cs, cs_ref)         # the carrier's own result
    assert torch.equal(dy, dy_alone)                                 # every element as the stand-alone pass writes it
    assert float(amax) == float(dy[:rows, :cols].abs().max()) == amax_alone
    assert bool((dy[:, cols:] == PAD).all()) and bool((dy[rows:] == PAD).all())
    return used


@pytest.mark.parametrize("shape", list(PLANNED))
def test_planned_period(lib, shape):
    """(a) the plan: the largest of 4, 2, 1 at which the launch's waves still reach every item."""
    assert _check(lib, *shape, 0) == PLANNED[shape]


@pytest.mark.parametrize("period", [1, 2, 4])
@pytest.mark.parametrize("shape", list(PLANNED) + FORCED_ONLY)
def test_forced_period(lib, shape, period):
    """(b) every period on every shape: an item pending when the k-loop ends (P = 9995: 17 k-tiles in the last
    split), period x items beyond the k-loop (the drain finishes the job), waves without an item (rows = 5)."""
    assert _check(lib, *shape, period) == period


@pytest.mark.parametrize("period", [0, 1, 2, 4])
def test_short_last_split(lib, period):
    """(c) P = 8192 is the smallest the transposed-read core accepts, and its splits have 32 k-tiles (the shapes
    above): the plan keeps at least 480 rows in every split but the last, so no P gives a side job whole splits
    of fewer than 4 k-tiles.  The last split can be that short: at P = 19969 it is one row, a k-loop of one
    k-tile that issues an item and leaves it pending.  Planned: 4993 groups for 320 waves x 32 k-tiles: 2."""
    assert _check(lib, 19969, 19969, 64, period) == (period or 2)


@pytest.mark.parametrize("shape", list(PLANNED))
def test_planned_period_bn_relu(lib, shape):
    """(d) the same plan under the <1, true> carrier (BN+ReLU on B)."""
    assert _check(lib, *shape, 0, bn=True) == PLANNED[shape]


@pytest.mark.parametrize("shape", list(PLANNED) + FORCED_ONLY)
def test_forced_period_4_bn_relu(lib, shape):
    assert _check(lib, *shape, 4, bn=True) == 4


def test_bad_period_is_an_error(lib):
    a, b, qa, qb, dy0, z, ka, kb, kc = _reference(lib, 8192, 5, 64, False)[:9]
    nb = lib.prh_test_gemm_tn_side_workspace_bytes(8192, MO, NI)
    ws = torch.empty(nb, dtype=torch.uint8, device="cuda")
    c = torch.empty(MO, NI, device="cuda")
    amax = torch.empty(1, device="cuda")
    rc = lib.prh_test_gemm_tn_side_ex(_p(a), _p(b), _p(c), None, 8192, MO, NI, None, None, _p(dy0.clone()), LD, _p(z), LD,
                                      _p(ka), _p(kb), _p(kc), 5, 64, 1, 3, None, _p(amax), _p(ws), nb, 0, None)
    assert rc != 0 and b"period" in lib.prh_last_error()
