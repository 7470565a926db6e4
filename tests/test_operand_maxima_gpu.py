"""Every producer of an "operand maximum" of the split-fp16 GEMM cores, pinned by value.

The default GEMM mode (3, split-fp16) places each operand by a power-of-two scale taken from a
device scalar, its largest magnitude.  Too small by more than 4x and the fp16 planes overflow;
too large and the small entries lose a bit per factor of two.  The scalar is a by-product of
seven different kernels; the end-to-end gates on randn-like data notice neither a maximum that
is 2^8 too large nor a stale one.  A maximum does not depend on the order of reduction, so
"equals" here is == on the fp32 value unless a margin is derived in the test's docstring.
"""
import ctypes as C
import gc

import numpy as np
import pytest
import torch

from conftest import maxdiff, rel_l2
from oracle import linerefine_oracle as O
from oracle import procedural as P

pytestmark = pytest.mark.gpu

ERR_ARG, ERR_WORKSPACE = -1, -2
ABSMAX_MAX_BLOCKS = 2048          # csrc/prh_gemm_s3.hpp


def _p(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def _st():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _dev():
    return torch.cuda.current_device()


def _set_mode(mode):
    from pointnet_refine_amd import _lib
    l = _lib.lib()
    old = l.prh_get_gemm_mode()
    assert l.prh_set_gemm_mode(mode) == 0
    return l, old


@pytest.fixture()
def lib():
    l, old = _set_mode(3)
    yield l
    l.prh_set_gemm_mode(old)


def _ws(lib):
    nb = lib.prh_operand_absmax_workspace_bytes()
    return torch.empty(nb, dtype=torch.uint8, device="cuda"), nb


def _absmax(lib, x, ld, rows, cols, out, ws, nb):
    return lib.prh_operand_absmax(_p(x), ld, rows, cols, _p(out), _p(ws), nb, _dev(), _st())


def _relu_mask(lib, dy, y, out, n, scale, amax, ws, nb):
    return lib.prh_relu_mask_absmax(_p(dy), _p(y), _p(out), n, C.c_float(scale), _p(amax), _p(ws), nb, _dev(), _st())


def _f32(v):
    return float(np.float32(v))


# ------------------------------------------------------------------------------------------
# A. prh_operand_absmax against x.abs().max()
# ------------------------------------------------------------------------------------------
ABSMAX_SHAPES = [(1, 1, 1), (3, 5, 7),            # scalar path, cols % 4 != 0
                 (33, 4, 4),
                 (31, 256, 448),                  # vector path, pad columns
                 (129, 260, 260),                 # 65 column vectors: a thread's second column trip
                 (65537, 8, 12),                  # one row past ABSMAX_MAX_BLOCKS * 32: the grid clamps, the row loop strides
                 (1000, 1984, 1984),
                 (5, 6, 8)]                       # cols % 4 != 0 with an aligned ld


@pytest.mark.parametrize("rows,cols,ld", ABSMAX_SHAPES)
def test_operand_absmax_finds_a_planted_maximum_anywhere(lib, rows, cols, ld):
    """randn operand, pad columns (ld > cols) full of 1e30 and NaN that must never be read, and
    the unique maximum -50 planted at the corners, at the end of the vector part of the last row
    (and the first scalar-tail column after it) and at one random position."""
    g = torch.Generator().manual_seed(rows * 31 + cols * 7 + ld)
    buf = torch.empty(rows, ld)
    buf[:, :cols] = torch.randn(rows, cols, generator=g)
    if ld > cols:
        buf[:, cols::2] = 1e30
        buf[:, cols + 1::2] = float("nan")
    x = buf.cuda()
    ws, nb = _ws(lib)
    out = torch.full((1,), float("nan"), device="cuda")
    ref = buf[:, :cols].abs().max()
    assert float(ref) < 50.0
    assert _absmax(lib, x, ld, rows, cols, out, ws, nb) == 0
    assert float(out) == float(ref)
    pos = [(0, 0), (0, cols - 1), (rows - 1, 0), (rows - 1, cols - 1)]
    cv = (cols // 4) * 4 - 1
    if cv >= 0:
        pos.append((rows - 1, cv))
        if cv + 1 < cols:
            pos.append((rows - 1, cv + 1))
    pos.append((int(torch.randint(rows, (1,), generator=g)), int(torch.randint(cols, (1,), generator=g))))
    for r, c in pos:
        keep = float(buf[r, c])
        x[r, c] = -50.0
        out.fill_(float("nan"))
        assert _absmax(lib, x, ld, rows, cols, out, ws, nb) == 0
        assert float(out) == 50.0, (r, c, float(out))
        x[r, c] = keep


def test_operand_absmax_edge_values_and_errors(lib):
    """rows = 0 and an all-zero operand give 0; fp32 denormals come back exactly; a NaN inside the
    operand is DROPPED (the kernels reduce with fmaxf, which returns its other argument), so the
    result is the maximum of the finite entries; ld < cols and cols = 0 are argument errors.

    Workspace: prh_operand_absmax_workspace_bytes() = 4 * ABSMAX_MAX_BLOCKS for the partials + 256
    bytes of alignment slack.  The advertised size is accepted; one byte less than the partials
    need (from an aligned base) is PRH_ERR_WORKSPACE."""
    from pointnet_refine_amd import ops
    ws, nb = _ws(lib)
    assert nb == 4 * ABSMAX_MAX_BLOCKS + 256
    out = torch.full((1,), float("nan"), device="cuda")
    x = torch.randn(64, 8, device="cuda")
    assert _absmax(lib, x, 8, 0, 8, out, ws, nb) == 0
    assert float(out) == 0.0
    for rows, cols in ((33, 4), (3, 5)):
        out.fill_(float("nan"))
        z = torch.zeros(rows, cols, device="cuda")
        z[rows // 2, cols - 1] = -0.0
        assert _absmax(lib, z, cols, rows, cols, out, ws, nb) == 0
        assert float(out) == 0.0
        # denormals: 1e-40 .. 7e-40, the largest one negative
        d = (torch.arange(rows * cols, dtype=torch.float32).reshape(rows, cols) % 7 + 1) * 1e-40
        d[rows - 1, cols - 1] = -9.5e-40
        assert 0.0 < float(d.abs().max()) < 1.1754944e-38
        out.fill_(float("nan"))
        assert _absmax(lib, d.cuda(), cols, rows, cols, out, ws, nb) == 0
        assert float(out) == float(d.abs().max()) == _f32(9.5e-40)
        # NaN inside the operand
        v = torch.randn(rows, cols, generator=torch.Generator().manual_seed(rows))
        v[0, 0] = float("nan")
        v[rows - 1, cols - 1] = float("nan")
        v[rows // 2, 1] = -7.25
        out.fill_(float("nan"))
        assert _absmax(lib, v.cuda(), cols, rows, cols, out, ws, nb) == 0
        assert float(out) == 7.25
    assert _absmax(lib, x, 7, 64, 8, out, ws, nb) == ERR_ARG
    assert _absmax(lib, x, 8, 64, 0, out, ws, nb) == ERR_ARG
    assert _absmax(lib, x, 8, 64, 8, out, ws, 4 * ABSMAX_MAX_BLOCKS - 1) == ERR_WORKSPACE
    assert _absmax(lib, x, 8, 64, 8, out, ws, nb) == 0
    t = torch.randn(257, 64, generator=torch.Generator().manual_seed(5))
    t[200, 63] = -9.0
    got = ops.operand_absmax(t.cuda())
    assert got.shape == (1,) and float(got) == float(t.abs().max()) == 9.0


# ------------------------------------------------------------------------------------------
# B. one workspace, one stream, large and small operands in turn
# ------------------------------------------------------------------------------------------
def test_one_workspace_measures_large_and_small_operands_in_turn(lib):
    """The per-block partials live in one workspace that every measurement rewrites, and the
    one-block reduction tends to land on the CU that reduced the previous one: it must read the
    partials of THIS launch (agent-scope loads in absmax_final_kernel).  X (65537 x 8, maximum
    3e4, 2048 partials) and Y (33 x 4, maximum 2e-3, 2 partials) alternate through one workspace
    on one stream without any synchronisation; four different slots, then one slot written
    twice.  Then the same with prh_relu_mask_absmax, which shares the workspace layout.  The
    sequence runs once: it checks the documented loads, it is not a stress run."""
    g = torch.Generator().manual_seed(3)
    X = (torch.rand(65537, 8, generator=g) * 2 - 1) * 1e4
    X[65536, 7] = -3e4
    Y = (torch.rand(33, 4, generator=g) * 2 - 1) * 1e-3
    Y[32, 0] = 2e-3
    X, Y = X.cuda(), Y.cuda()
    n = 1024 * 4 * 64
    dy = (torch.rand(n, generator=g) * 2 - 1) * 1e-3
    dy[n - 1] = -4e-3
    yv = torch.ones(n)
    dy, yv = dy.cuda(), yv.cuda()
    masked = torch.empty_like(dy)
    ws, nb = _ws(lib)
    out = torch.full((10,), float("nan"), device="cuda")
    torch.cuda.synchronize()
    seq = [(X, 0), (Y, 1), (X, 2), (Y, 3), (X, 4), (Y, 4)]
    for t, slot in seq:
        assert _absmax(lib, t, t.shape[1], t.shape[0], t.shape[1], out[slot:], ws, nb) == 0
    # 64 partials of the masked pass against 2048 of X
    assert _absmax(lib, X, 8, 65537, 8, out[5:], ws, nb) == 0
    assert _relu_mask(lib, dy, yv, masked, n, 1.0, out[6:], ws, nb) == 0
    assert _absmax(lib, X, 8, 65537, 8, out[7:], ws, nb) == 0
    assert _relu_mask(lib, dy, yv, masked, n, 1.0, out[8:], ws, nb) == 0
    assert _absmax(lib, Y, 4, 33, 4, out[9:], ws, nb) == 0
    got = out.cpu().tolist()
    big, small, mid = _f32(3e4), _f32(2e-3), _f32(4e-3)
    assert got == [big, small, big, small, small, big, mid, big, mid, small], got


# ------------------------------------------------------------------------------------------
# D. prh_relu_mask_absmax
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scale", [1.0, 1.0 / (1.0 - 0.1)], ids=["plain", "dropout0.1"])
@pytest.mark.parametrize("n", [4, 1024, 4100, 1024 * 4 * 2048 + 4])     # the last: one float4 past what 2048 blocks cover in one trip
def test_relu_mask_absmax(lib, n, scale):
    """out = y > 0 ? dy * scale : 0 bitwise (one fp32 multiply) and amax = max|out|.  y holds exact
    zeros, -0.0 and negative values: all masked (the test is y > 0).  The three largest |dy| sit
    on one masked position of each kind and must not count; the largest survivor (negative) is
    the last element."""
    g = torch.Generator(device="cuda").manual_seed(n % 1000 + 1)
    y = torch.randn(n, device="cuda", generator=g)
    dy = torch.randn(n, device="cuda", generator=g)
    y[0::3] = 0.0
    y[1::7] = -0.0
    y[2] = -3.0
    y[n - 1] = 0.5
    dy[0], dy[1], dy[2] = 1e6, -2e6, 3e6
    dy[n - 1] = -100.0
    s32 = _f32(scale)
    ref = torch.where(y > 0, dy * s32, torch.zeros_like(dy))
    ws, nb = _ws(lib)
    out = torch.full((n,), float("nan"), device="cuda")
    amax = torch.full((1,), float("nan"), device="cuda")
    assert _relu_mask(lib, dy, y, out, n, s32, amax, ws, nb) == 0
    assert torch.equal(out.view(torch.int32), ref.view(torch.int32))
    assert float(amax) == float(ref.abs().max()) == float(np.float32(100.0) * np.float32(s32))
    assert _relu_mask(lib, dy, y, out, n + 2, s32, amax, ws, nb) == ERR_ARG


# ------------------------------------------------------------------------------------------
# C. the training encoder's slots op_amax[0..6]
# ------------------------------------------------------------------------------------------
BN_KEYS = ["bn1.weight", "bn2.weight", "bn3.weight", "bn4.weight", "bn5.weight", "fusion.1.weight"]
BOOST_CHANNEL = 1          # the negative-gamma channel of every layer whose |gamma| is multiplied by 8
CTX_OFFSET = 100.0         # gamma case 3: added to input channels 0..2
BIAS_OFFSET = 30.0         # case 4: pre-BatchNorm bias -30 on channels 2 and 3 of conv1..4 (all gamma positive)


def _encoder_inputs(B, N, out_dim, case, seed=9, offset=None):
    """state dict + context of gamma case 1 (as generated, all gamma positive), 2 (every second
    channel of every BatchNorm negated, |gamma| of channel BOOST_CHANNEL times 8), 3 (case 2
    plus CTX_OFFSET, or `offset`, on input channels 0..2: column means far from zero) or 4 (case 1
    plus a pre-BatchNorm bias of -BIAS_OFFSET on channels 2 and 3 of conv1..4)."""
    sd = P.encoder_state_dict(4, out_dim, seed=seed)
    ctx, _, _ = P.synth_batch(B, N, 4, 32, seed=31)
    if case in (2, 3):
        for k in BN_KEYS:
            sd[k][1::2] *= -1.0
            sd[k][BOOST_CHANNEL] *= 8.0
    if case == 3:
        ctx[..., 0:3] += CTX_OFFSET if offset is None else offset
    if case == 4:
        for k in range(1, 5):
            sd[f"conv{k}.bias"][2:4] = -BIAS_OFFSET
    return sd, ctx


def _encoder(sd, out_dim):
    from pointnet_refine_amd.model import MultiScalePointNetEncoder
    m = MultiScalePointNetEncoder(in_channel=4, out_dim=out_dim)
    m.load_state_dict(sd, strict=True)
    return m.cuda().train()


def _ulp32(v):
    return float(np.spacing(np.float32(abs(v))))


def _check_slots(fused, out_dim, want_negative):
    """coef[4][0..6] against an fp64 recomputation from the saved fp32 z / scale / shift."""
    saved = fused.grad_fn.saved_tensors          # x, z_cat, z_fus, gate, coef, ...
    z_cat, z_fus, coef = saved[1], saved[2], saved[4]
    widths = [64, 128, 256, 512, out_dim]
    cat = sum(widths)
    assert z_cat.shape[1] == cat and coef.shape == (5, cat + out_dim)
    slots = coef[4, :7].cpu().tolist()
    blocks = [(z_cat[:, sum(widths[:l]):sum(widths[:l + 1])], sum(widths[:l]), widths[l]) for l in range(5)]
    blocks.append((z_fus, cat, out_dim))
    for l, (z, off, w) in enumerate(blocks):
        sc, sh = coef[0, off:off + w].double(), coef[1, off:off + w].double()
        per_ch = torch.relu(z.double() * sc + sh).amax(dim=0)
        a = float(per_ch.max())
        ch = int(per_ch.argmax())
        slot = slots[l] if l < 5 else slots[6]
        print(f"layer {l}: slot {slot!r} fp64 {a!r} arg-max channel {ch} scale {float(sc[ch]):+.4f}")
        assert a > 0.0
        if want_negative:       # the maximum sits at a column MINIMUM, or the case tests nothing
            assert float(sc[ch]) < 0.0, (l, ch)
        assert abs(slot - a) <= _ulp32(a), (l, slot, a)
    assert slots[5] == max(slots[0:5])
    assert slots[6] >= float(fused.abs().max())
    assert all(np.isfinite(slots))
    return slots


ENC_SIZES = [(2, 100),       # small cores only
             (3, 171),       # P = 513: one row past a tile
             (5, 1999)]      # P = 9995: split-fp16 NT cores, nothing aligned


@pytest.mark.parametrize("case", [1, 2, 3, 4], ids=["gamma+", "gamma-", "gamma-,offset", "bias"])
@pytest.mark.parametrize("B,N", ENC_SIZES)
def test_encoder_slots_equal_the_activation_maxima(lib, B, N, case):
    """op_amax[l] = max relu(z_l * scale_l + shift_l) comes from the per-row-block column maxima AND
    minima of the statistics epilogue.  The kernel rounds one fmaf of three fp32 inputs; the fp64
    recomputation of the same inputs rounds at most once more: margin one fp32 ulp.  With a
    negative gamma (case 2) the maximum sits at a column minimum; with column means far from zero
    (case 3: +100 on the input coordinates; case 4: all gamma positive, a pre-BatchNorm bias of
    -30 on two channels of conv1..4, which moves the means without costing the fp32 inputs any
    bits) a padded tile row (z = 0) that entered the recorded extrema would inflate the slot by
    orders of magnitude.  In cases 3 and 4 the backward runs too and every gradient is finite:
    the split-fp16 wgrad reads relu(BN(z)) of the rows beyond P as relu(shift), far above the
    operand maximum."""
    sd, ctx = _encoder_inputs(B, N, 1024, case)
    m = _encoder(sd, 1024)
    x = ctx.cuda().requires_grad_(True)
    gf, fused = m.forward_pointmajor(x, True)
    _check_slots(fused, 1024, want_negative=case in (2, 3))
    if case >= 3:
        (gf.sum() + fused.sum()).backward()
        assert bool(torch.isfinite(x.grad).all())
        for k, v in m.named_parameters():
            assert bool(torch.isfinite(v.grad).all()), k


def _vs_oracle(sd, ctx, out_dim, seed):
    """forward + backward with upstream gradients on both outputs against the fp32 CPU oracle, at
    the gates of test_encoder_train_ragged_large_vs_oracle_on_split_cores."""
    import re
    B, N = ctx.shape[0], ctx.shape[1]
    r = np.random.default_rng(seed)
    up_g = torch.from_numpy(r.normal(0, 1, (B, 2 * out_dim)).astype(np.float32))
    up_f = torch.from_numpy(r.normal(0, 1, (B, N, out_dim)).astype(np.float32))
    m = _encoder(sd, out_dim)
    x = ctx.cuda().requires_grad_(True)
    gf, fu = m.forward_pointmajor(x, True)
    slots = _check_slots(fu, out_dim, want_negative=bool((sd["bn1.weight"] < 0).any()))
    ((gf * up_g.cuda()).sum() + (fu * up_f.cuda()).sum()).backward()
    p = O.as_params(sd, requires_grad=True)
    ox = ctx.clone().requires_grad_(True)
    o_g, o_f = O.encoder_forward(p, ox, "", True, {})
    ((o_g * up_g).sum() + (o_f * up_f).sum()).backward()
    fwd = max(maxdiff(gf, o_g), maxdiff(fu, o_f))
    dx = rel_l2(ox.grad, x.grad)
    rels = {}
    for k, v in m.named_parameters():
        assert bool(torch.isfinite(v.grad).all()), k
        if re.search(r"(conv\d\.bias|fusion\.0\.bias)$", k):      # bias ahead of a BatchNorm: gradient is rounding noise
            continue
        rels[k] = rel_l2(p[k].grad.reshape(v.shape), v.grad)
    worst = max(rels, key=rels.get)
    print(f"forward maxdiff {fwd:.3e}, d_ctx rel-L2 {dx:.3e}, worst parameter {worst} {rels[worst]:.3e}")
    assert bool(torch.isfinite(x.grad).all())
    assert fwd < 1e-4
    assert dx < 5e-3
    assert rels[worst] < 1e-2, worst
    return slots


@pytest.mark.parametrize("case,offset", [(3, 2.0), (4, None)], ids=["gamma-,offset2", "bias"])
def test_encoder_far_means_vs_oracle_on_split_cores(lib, case, offset):
    """P = 5 x 1999 through forward and backward against the fp32 oracle.

    Case 3 with the input offset lowered from 100 to 2: fp32 BatchNorm itself loses the room at
    100.  fp32 oracle against fp64 oracle on these inputs (forward max-abs / d_ctx rel-L2 / worst
    parameter rel-L2; half gates 5e-5 / 2.5e-3 / 5e-3):
        offset 100: 8.4e-4 / 7.0e-3 / 8.6e-3      offset 32: 2.6e-4 / 5.6e-3 / 7.9e-3
        offset 16:  1.6e-4 / 3.2e-3 / 3.4e-3      offset 8:  6.8e-5 / 2.8e-3 / 3.5e-3
        offset 4:   4.8e-5 / 4.9e-4 / 1.7e-3      offset 2:  3.6e-5 / 2.2e-4 / 5.4e-4
        offset 0:   3.7e-5 / 7.4e-4 / 2.0e-3  (the |gamma| x 8 channels set this floor)
    Case 4 (pre-BatchNorm bias -30, all gamma positive): 1.6e-5 / 6.1e-4 / 1.3e-3 (bias -100:
    3.8e-5 / 3.1e-3 / 3.3e-3, over half the d_ctx gate).  Its conv1 channels 2 and 3 have
    shift = 52 and 37 against an activation maximum of 7.3: relu(shift) times the operand's
    power-of-two scale 2^11 is beyond fp16, which is what a row past P of the wgrad's B operand
    holds (NaN in conv2.weight's gradient before the clamp in relu_f16).
    The kernels against the fp32 oracle, as measured: case 3 4.8e-5 / 5.3e-4 / 1.7e-3, case 4
    2.2e-5 / 2.3e-3 / 2.1e-3."""
    sd, ctx = _encoder_inputs(5, 1999, 1024, case, offset=offset)
    _vs_oracle(sd, ctx, 1024, seed=6)


@pytest.mark.parametrize("case", [1, 2], ids=["gamma+", "gamma-"])
def test_encoder_wider_than_the_partial_buffer(lib, case):
    """out_dim = 2112: conv5 and the fusion layer are wider than the 2048 columns whose
    32-column blocks x 32 row slices fill act_amax_kernel's ABSMAX_MAX_BLOCKS partials in one trip.
    Slots 4 and 6 must still be written (and slot 5 be the maximum of written slots): P = 800
    gives 4 x 9 tiles of 256 >= 32, so nt_use_s3 holds for the fusion GEMM (K = 3072, N = 2112)
    and it reads its A scale from slot 5; context_proj reads slot 6.  Forward and backward
    against the fp32 oracle; fp32 oracle against fp64 oracle on these inputs (forward max-abs /
    d_ctx rel-L2 / worst parameter rel-L2): gamma+ 1.5e-5 / 7.6e-7 / 1.0e-6, gamma- 2.7e-5 /
    4.0e-4 / 1.6e-3, inside half of the gates 1e-4 / 5e-3 / 1e-2.  The kernels against the fp32
    oracle, as measured: gamma+ 1.7e-5 / 1.2e-6 / 2.0e-6, gamma- 6.1e-5 / 1.0e-3 / 1.7e-3."""
    B, N, od = 2, 400, 2112
    assert lib.prh_linear_uses_operand_maxima(B * N, 64 + 128 + 256 + 512 + od, od) == 1
    sd, ctx = _encoder_inputs(B, N, od, case)
    # poison the caching allocator's free blocks: a slot nobody writes then holds NaN, not a
    # plausible number left by an earlier test
    junk = torch.full((5, 960 + 2 * od), float("nan"), device="cuda")
    del junk
    _vs_oracle(sd, ctx, od, seed=8)


# ------------------------------------------------------------------------------------------
# E. attention backward: kv_amax_part and the hint that carries it to the K/V projections
# ------------------------------------------------------------------------------------------
H, CH = 8, 256
USED = (0, 2, 5)


def _arena_run(B, M, N, seed, boost=None, proj=False):
    """Three of six attention blocks against wide K/V buffers with the gradient arena.  proj: K/V come
    from ops.linear (rows B*N, 256 -> 6*256).  Returns the arena's per-wave maxima (grabbed when
    the token's gradient arrives, i.e. after every attention backward and before KVTokenFn's)."""
    from pointnet_refine_amd import ops
    g = torch.Generator().manual_seed(seed)
    q = [torch.randn(B, M, CH, generator=g).cuda().requires_grad_(True) for _ in range(6)]
    up = [torch.randn(B, M, CH, generator=g).cuda() for _ in range(6)]
    r = {}
    if proj:
        r["mem"] = torch.randn(B, N, CH, generator=g).cuda().requires_grad_(True)
        r["wk"] = (torch.randn(6 * CH, CH, generator=g) / 16).cuda().requires_grad_(True)
        r["wv"] = (torch.randn(6 * CH, CH, generator=g) / 16).cuda().requires_grad_(True)
        r["bk"] = torch.randn(6 * CH, generator=g).cuda().requires_grad_(True)
        r["bv"] = torch.randn(6 * CH, generator=g).cuda().requires_grad_(True)
        ka, va = ops.linear(r["mem"], r["wk"], r["bk"]), ops.linear(r["mem"], r["wv"], r["bv"])
    else:
        ka = torch.randn(B, N, 6 * CH, generator=g).cuda().requires_grad_(True)
        va = torch.randn(B, N, 6 * CH, generator=g).cuda().requires_grad_(True)
    token, arena = ops.kv_token(ka, va, CH)
    grabbed = []
    token.register_hook(lambda gr: grabbed.append(arena.part))
    outs = [ops.attention_block(q[i], ka, va, token, arena, i, H) for i in USED]
    loss = 0.0
    for o, i in zip(outs, USED):
        loss = loss + (o * up[i]).sum() * (boost[1] if (boost and boost[0] == i) else 1.0)
    r.update(ka=ka, va=va, loss=loss, grabbed=grabbed, arena=arena)
    return r


ATTN_SHAPES = [(2, 32, 200), (3, 20, 33),
               (2, 45, 130),        # M > 32: dK / dV accumulate over query tiles
               (4, 32, 256)]        # key-split mode of the fp16 kernels: B x H <= 1024 and N >= 128


@pytest.mark.parametrize("B,M,N", ATTN_SHAPES)
@pytest.mark.parametrize("mode", [3, 0], ids=["split16", "fp32"])
def test_attention_backward_records_the_kv_gradient_maxima(mode, B, M, N):
    """part[i] (per-wave maxima of block i) bounds max|dV_i| / max|dK_i| from above, equals them
    when M <= 32 (every element is stored once), is exactly zero for unused blocks, and only the
    row of a block whose upstream gradient is scaled by 1e3 moves (by 1e3, to the rounding of the
    scaled products: 1e-5 relative).  For M > 32 the kernel takes the maximum over running sums:
    only >= is asserted and the ratio printed (measured at (2, 45, 130), both modes: between
    1.0000 and 1.0788 for dV, 1.0000 and 1.0048 for dK)."""
    l, old = _set_mode(mode)
    try:
        rows = {}
        for tag, boost in (("base", None), ("x1e3", (2, 1e3))):
            r = _arena_run(B, M, N, seed=B * 100 + M, boost=boost)
            r["loss"].backward()
            assert len(r["grabbed"]) == 1 and r["grabbed"][0] is not None
            part = r["grabbed"][0]
            assert part.shape == (6, B * H, 2) and r["arena"].part is None
            pm = part.amax(dim=1).cpu()            # [block][dV, dK]
            dv, dk = r["va"].grad, r["ka"].grad
            for i in range(6):
                tv = float(dv[..., i * CH:(i + 1) * CH].abs().max())
                tk = float(dk[..., i * CH:(i + 1) * CH].abs().max())
                bv, bk = float(pm[i, 0]), float(pm[i, 1])
                if i not in USED:
                    assert bv == 0.0 and bk == 0.0 and tv == 0.0 and tk == 0.0
                    assert float(part[i].abs().max()) == 0.0
                    continue
                assert tv > 0.0 and tk > 0.0
                assert bv >= tv and bk >= tk, (i, bv, tv, bk, tk)
                if M <= 32:
                    assert bv == tv and bk == tk, (i, bv, tv, bk, tk)
                else:
                    print(f"mode {mode} block {i} {tag}: bound / true dV {bv / tv:.4f} dK {bk / tk:.4f}")
            rows[tag] = pm
        for i in USED:
            if i == 2:
                ratio = rows["x1e3"][i] / rows["base"][i]
                assert float((ratio / 1e3 - 1).abs().max()) < 1e-5, ratio
            else:
                assert torch.equal(rows["x1e3"][i], rows["base"][i])
    finally:
        l.prh_set_gemm_mode(old)


@pytest.mark.parametrize("M", [32, 45])
def test_kv_gradient_hint_equals_the_measured_maximum(lib, M):
    """K/V projections of 8 x 1024 rows, 256 -> 1536: their dgrad (32 x 1 tiles, K = 1536) and wgrad
    (P >= 8192) run on the split-fp16 cores and read max|dy|.  With the hint from the attention
    backward and with the hint dropped before the projections' backward (measured path) the
    projection gradients are bitwise equal for M <= 32 (hint = measurement) and within 1e-6
    rel-L2 for M > 32 (an upper bound).  Nothing is left in ops._DY_AMAX afterwards."""
    from pointnet_refine_amd import ops
    B, N = 8, 1024
    assert lib.prh_linear_uses_operand_maxima(B * N, CH, 6 * CH) == 1
    res = []
    for drop in (False, True):
        ops._DY_AMAX.clear()
        r = _arena_run(B, M, N, seed=77, proj=True)
        seen = []

        def hook(gr, drop=drop, seen=seen):
            h = ops._DY_AMAX.get(id(gr))
            seen.append(h is not None and h[2]() is gr)
            if drop:
                ops._DY_AMAX.clear()

        r["ka"].register_hook(hook)
        r["va"].register_hook(hook)
        r["loss"].backward()
        assert len(ops._DY_AMAX) == 0
        if not drop:
            assert seen == [True, True]        # each projection's dy arrives with its own hint
        res.append([r[k].grad.clone() for k in ("mem", "wk", "wv", "bk", "bv")])
    for name, a, b in zip(("d_mem", "dWk", "dWv", "dbk", "dbv"), res[0], res[1]):
        assert bool(torch.isfinite(a).all()), name
        if M <= 32:
            assert torch.equal(a, b), name
        else:
            e = rel_l2(b, a)
            print(f"{name}: hint vs measured rel-L2 {e:.3e}")
            assert e < 1e-6, name


def test_a_hint_nobody_consumed_is_not_taken_by_another_tensor(lib):
    """K/V of an arena graph that do not come from ops.linear: nothing pops the two hints.  After
    everything is freed, an unrelated Linear's backward receives a dy of the old dK's shape, 1e4
    times larger - and, the allocator willing, at the old dK's address.  A scale taken from the
    stale hint would overflow the fp16 planes (with hints keyed by address it did: non-finite
    gradients; they are keyed by tensor identity and die with their tensor)."""
    from pointnet_refine_amd import ops
    B, M, N = 8, 45, 1024
    r = _arena_run(B, M, N, seed=5)
    r["loss"].backward()
    old_max = float(r["ka"].grad.abs().max())
    old_ptrs = {r["ka"].grad.data_ptr(), r["va"].grad.data_ptr()}
    shape = tuple(r["ka"].grad.shape)
    del r
    gc.collect()
    g = torch.Generator().manual_seed(9)
    x = torch.randn(B, N, CH, generator=g).cuda().requires_grad_(True)
    w = (torch.randn(6 * CH, CH, generator=g) / 16).cuda().requires_grad_(True)
    b = torch.randn(6 * CH, generator=g).cuda().requires_grad_(True)
    y = ops.linear(x, w, b)
    assert tuple(y.shape) == shape
    cands = [torch.empty(shape, device="cuda") for _ in range(6)]       # the freed blocks are the best fit
    dy = next((c for c in cands if c.data_ptr() in old_ptrs), cands[0])
    del cands
    print("dy landed on a freed gradient's address:", dy.data_ptr() in old_ptrs)
    dy.copy_(torch.randn(shape, generator=g) * (1e4 * old_max))
    y.backward(gradient=dy)
    x64, w64, dy64 = x.detach().double(), w.detach().double(), dy.double()
    refs = {"dx": dy64 @ w64, "dw": dy64.reshape(-1, 6 * CH).t() @ x64.reshape(-1, CH), "db": dy64.sum(dim=(0, 1))}
    for name, got in (("dx", x.grad), ("dw", w.grad), ("db", b.grad)):
        assert bool(torch.isfinite(got).all()), name
        e = rel_l2(refs[name], got)
        print(f"{name} rel-L2 vs fp64 {e:.3e}")
        assert e < 1e-5, name


# ------------------------------------------------------------------------------------------
# F. maxima handed to a launch against maxima the launch measures
# ------------------------------------------------------------------------------------------
def _lin_fwd(lib, x, w, b, xa, wa):
    rows, k = x.shape
    n = w.shape[0]
    nb = lib.prh_linear_forward_workspace_bytes(rows, k, n)
    ws = torch.empty(nb, dtype=torch.uint8, device="cuda")
    y = torch.full((rows, n), float("nan"), device="cuda")
    assert lib.prh_linear_forward_full(_p(x), k, _p(w), _p(b), None, 0, _p(y), rows, k, n, 0, _p(xa), _p(wa),
                                       C.c_float(0.0), 0, _p(ws), nb, _dev(), _st()) == 0
    return y


def _lin_bwd(lib, x, w, dy, xa, da, wa):
    rows, k = x.shape
    n = w.shape[0]
    nb = lib.prh_linear_backward_workspace_bytes(rows, k, n)
    ws = torch.empty(nb, dtype=torch.uint8, device="cuda")
    dx = torch.full((rows, k), float("nan"), device="cuda")
    dw = torch.full((n, k), float("nan"), device="cuda")
    db = torch.full((n,), float("nan"), device="cuda")
    assert lib.prh_linear_backward_full(_p(x), k, _p(w), _p(dy), _p(dx), _p(dw), _p(db), rows, k, n, _p(xa), _p(da),
                                        _p(wa), _p(ws), nb, _dev(), _st()) == 0
    return dx, dw, db


def _measure(lib, t):
    ws, nb = _ws(lib)
    out = torch.full((1,), float("nan"), device="cuda")
    assert _absmax(lib, t, t.shape[1], t.shape[0], t.shape[1], out, ws, nb) == 0
    return out


def _operands(rows, k, n, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.rand(rows, k, generator=g) * 2 - 1
    x[rows - 1, k - 1] = -1.0                     # max|x| = 1.0 exactly
    w = (torch.rand(n, k, generator=g) * 2 - 1) * 0.25
    w[n // 2, 3] = 0.25                           # max|w| = 0.25 exactly
    b = torch.randn(n, generator=g)
    dy = torch.randn(rows, n, generator=g)
    return x.cuda(), w.cuda(), b.cuda(), dy.cuda()


def test_linear_forward_supplied_maxima_equal_measured_ones(lib):
    """rows = 2049, k = 64, n = 1024 (9 x 4 tiles): the smallest Linear on the split-fp16 NT core.
    NULL maxima (the launch measures) and the prh_operand_absmax results give bitwise the same y;
    so do maxima 1.4x larger inside the same binade (pow2_scale reads the exponent only).  A
    bound 2^4 too large, and operands at 1e-12 / 1e10 through the supplied path, stay at the
    1e-6 rel-L2 gate of test_split16_operand_scales against fp64."""
    rows, k, n = 2049, 64, 1024
    assert lib.prh_linear_uses_operand_maxima(rows, k, n) == 1
    x, w, b, _ = _operands(rows, k, n, 21)
    xa, wa = _measure(lib, x), _measure(lib, w)
    assert float(xa) == 1.0 and float(wa) == 0.25
    y0 = _lin_fwd(lib, x, w, b, None, None)
    assert bool(torch.isfinite(y0).all())
    assert torch.equal(y0, _lin_fwd(lib, x, w, b, xa, wa))
    assert torch.equal(y0, _lin_fwd(lib, x, w, b, xa * 1.4, wa * 1.4))
    ref = x.double() @ w.double().t() + b.double()
    assert rel_l2(ref, y0) < 1e-6
    e = rel_l2(ref, _lin_fwd(lib, x, w, b, xa * 16, wa * 16))
    print(f"maxima 2^4 too large: rel-L2 {e:.3e}")
    assert e < 1e-6
    xs, wsm = x * 1e-12, w * 1e10
    e = rel_l2(xs.double() @ wsm.double().t() + b.double(), _lin_fwd(lib, xs, wsm, b, _measure(lib, xs), _measure(lib, wsm)))
    print(f"operands at 1e-12 / 1e10, supplied maxima: rel-L2 {e:.3e}")
    assert e < 1e-6


@pytest.mark.parametrize("rows,k,n", [(2049, 64, 1024),      # the forward's shape
                                      (8200, 256, 512)])     # dgrad (33 x 1 tiles) and wgrad (P >= 8192) on the split-fp16 cores too
def test_linear_backward_supplied_maxima_equal_measured_ones(lib, rows, k, n):
    """dx, dw and db with all three maxima NULL are bitwise equal to the call that is handed them."""
    assert lib.prh_linear_uses_operand_maxima(rows, k, n) == 1
    x, w, _, dy = _operands(rows, k, n, 22)
    xa, wa, da = _measure(lib, x), _measure(lib, w), _measure(lib, dy)
    a = _lin_bwd(lib, x, w, dy, None, None, None)
    b = _lin_bwd(lib, x, w, dy, xa, da, wa)
    refs = (dy.double() @ w.double(), dy.double().t() @ x.double(), dy.double().sum(0))
    for name, u, v, ref in zip(("dx", "dw", "db"), a, b, refs):
        assert torch.equal(u, v), name
        assert rel_l2(ref, u) < 1e-6, name
