"""Every attention kernel the library can launch, called at the C ABI and compared with the fp64 reference of
tests/_attn_ref.py on the operands AS STORED: prh_attn_forward / prh_attn_backward on the fp32 core (mode 0:
attn_fwd_kernel / attn_bwd_kernel) and on the split-fp16 core (mode 3: attn16_*_kernel<0>), and prh_attn_forward_kv16 /
prh_attn_backward_kv16 (mode 4: attn16_*_kernel<0, true>, K / V and dK / dV in bf16).  K / V are rounded to bf16 for
all three, so one reference serves them and what is left is each kernel's own fp32-level arithmetic - plus, in bf16
storage, the one rounding per query tile of dK / dV, which has a bound that follows from the format.

The shapes are the smallest that select each launch geometry of attn_forward / attn_backward (csrc/prh_lib.hip): one or
four heads per workgroup, the key split with 4, 5 and 8 waves, ragged key and query tiles, H = 4 / 8 / 12.  Outputs
start from a NaN sentinel and are compared whole, K / V sit in column block 0, 2 or 5 of a (B, N, 6 C) buffer whose
other blocks are NaN, and every gradient buffer has guard rows in front and behind.

Largest observed error / bound per storage over all cases and column blocks (MI355X; every test prints its own):
    fp32 K / V, mode 0:  o 0.056  lse 0.057  dq 0.037  dk 0.024  dv 0.024
    fp32 K / V, mode 3:  o 0.044  lse 0.044  dq 0.022  dk 0.021  dv 0.522
    bf16 K / V, mode 4:  o 0.044  lse 0.044  dq 0.022  dk 0.940  dv 0.935
The two things that stand out have been looked into.  bf16 dK / dV near 0.94: one exact round-to-nearest of the fp64
reference itself uses the same 0.940 / 0.935 of the bound (printed as dk_rne / dv_rne) - just above a power of two the
rounding moves a value by 2^-8 of itself, the bound is 1.05 times that, and a case has ~10^6 elements; the kernels add
nothing visible to it.  dV of the split-fp16 core grows with the key count (0.07 at N = 128, 0.16 at 289, 0.52 at 1000;
the other quantities and the fp32 core do not): the backward's probabilities are normalised (~1 / N) and are split into
two fp16 planes without a scale, so the low plane runs into fp16's subnormals as N grows.  Within the gate at every key
count here and at the model's N = 1024.
"""
import ctypes as C
from dataclasses import dataclass
from functools import lru_cache

import pytest
import torch

import _attn_ref as R

pytestmark = pytest.mark.gpu

GATE = 2e-5                                  # tests/test_attention_gpu.py: maxdiff(o), rel_l2(dq), rel_l2(dk / dv)
STORAGES = {"fp32_mode0": (0, False), "fp32_mode3": (3, False), "bf16_mode4": (4, True)}
BLOCKS = (0, 2, 5)                           # column blocks of the wide buffers; 5 ends at the buffer's last byte
GUARD = 3                                    # sentinel rows in front of and behind every output buffer
SEED = 1234567
NAN32, NAN16 = 0x7FC00000, 0x7FC0


@dataclass(frozen=True)
class Case:
    name: str
    B: int
    H: int
    M: int
    N: int
    p: float = 0.0
    wide_q: bool = False       # q is the first half of a (B, M, 2 C) buffer
    twice: bool = False        # run forward and backward twice and compare bits


CASES = (
    [Case(f"plain_keytail_N{n}", 3, 8, 32, n) for n in (1, 31, 33, 127)] +
    [Case("plain_wideq_N33", 3, 8, 32, 33, wide_q=True)] +
    [Case(f"qtiles_M{m}_p{p}", 2, 8, m, 70, p) for m in (20, 45) for p in (0.0, 0.2)] +
    [Case("split4_N128", 2, 8, 32, 128), Case("split5_last2_N130", 2, 8, 32, 130), Case("split5_ragged_N289", 2, 8, 32, 289),
     Case("split8_N1000", 2, 8, 32, 1000, twice=True), Case("split8_N1000_p0.1", 2, 8, 32, 1000, 0.1, twice=True),
     Case("split_3qtiles_M70_N289", 1, 8, 70, 289), Case("nosplit_B129_N130", 129, 8, 32, 130, 0.1),
     Case("wpb4_B256", 256, 8, 32, 33, 0.1, twice=True), Case("H4", 3, 4, 32, 33), Case("H12", 3, 12, 32, 33),
     # B = 128 with H = 12 gives 384 workgroups' worth of heads, below the 512 at which four heads share a workgroup:
     # it runs one head per workgroup.  B = 171 (513) is the smallest batch that selects wpb = 4 with hpb = 3
     Case("H12_B128", 128, 12, 32, 33), Case("H12_wpb4_B171", 171, 12, 32, 33)])


def test_the_cases_select_the_launch_geometries_they_are_named_for():
    """The launch rules of attn_forward / attn_backward restated, so that a change of a threshold there does not
    silently turn these cases into repeats of one another."""
    def geometry(c, split_capable):
        wpb = 1 if c.B * (c.H // 4) < 512 else 4
        if split_capable and c.B * c.H <= 1024 and c.N >= 128:
            tiles = -(-c.N // 32)
            per_wave = -(-tiles // min(tiles, 8)) * 32
            return "split", -(-c.N // per_wave), per_wave
        return "plain", wpb, 0
    g = {c.name: geometry(c, True) for c in CASES}
    assert g["split4_N128"] == ("split", 4, 32) and g["split5_last2_N130"] == ("split", 5, 32)
    assert g["split5_ragged_N289"] == ("split", 5, 64) and g["split8_N1000"] == ("split", 8, 128)
    assert g["split_3qtiles_M70_N289"] == ("split", 5, 64)
    assert g["nosplit_B129_N130"] == ("plain", 1, 0) and g["wpb4_B256"] == ("plain", 4, 0)
    assert g["H12_wpb4_B171"] == ("plain", 4, 0) and g["H12_B128"] == ("plain", 1, 0)
    assert g["H12"] == ("plain", 1, 0) and g["H4"] == ("plain", 1, 0)
    assert all(geometry(c, False)[0] == "plain" for c in CASES)                      # mode 0 never splits


def _p(t, byte_offset=0):
    return C.c_void_p(t.data_ptr() + byte_offset)


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _sentinel(rows, width, dtype):
    """A (rows, width) view inside a buffer of NaN bits with GUARD rows on either side; returns (view, whole)."""
    if dtype == torch.float32:
        whole = torch.full((rows + 2 * GUARD, width), NAN32, dtype=torch.int32, device="cuda").view(torch.float32)
    else:
        whole = torch.full((rows + 2 * GUARD, width), NAN16, dtype=torch.int16, device="cuda").view(torch.bfloat16)
    return whole[GUARD:GUARD + rows], whole


def _is_sentinel(t):
    if t.dtype == torch.float32:
        return bool((t.contiguous().view(torch.int32) == NAN32).all())
    return bool((t.contiguous().view(torch.int16) == NAN16).all())


@pytest.fixture()
def lib_mode():
    """The library, with a setter for the GEMM mode that is undone afterwards."""
    from pointnet_refine_amd import _lib
    lib = _lib.lib()
    old = lib.prh_get_gemm_mode()

    def set_mode(m):
        assert lib.prh_set_gemm_mode(m) == 0
        return lib
    yield set_mode
    lib.prh_set_gemm_mode(old)


@lru_cache(maxsize=2)
def _reference(c):
    """Operands and fp64 results of a case, computed once on the GPU and shared by the three storages."""
    from pointnet_refine_amd import ops
    Cw, scale = 32 * c.H, 32.0 ** -0.5
    g = torch.Generator().manual_seed(c.B * 1000 + c.N + c.M)
    q = torch.randn(c.B, c.M, Cw, generator=g).cuda()
    k = torch.randn(c.B, c.N, Cw, generator=g).to(torch.bfloat16).cuda()
    v = torch.randn(c.B, c.N, Cw, generator=g).to(torch.bfloat16).cuda()
    up = torch.randn(c.B, c.M, Cw, generator=g).cuda()
    p32 = torch.tensor(c.p, dtype=torch.float32).item()      # the rate as the C ABI's float carries it
    keep = ops.attention_keep_mask(c.B, c.H, c.M, c.N, p32, SEED, device="cuda") if c.p > 0 else None
    o, lse = R.attn_ref(q, k, v, c.H, scale, keep, p32)
    dq, ck, cv = R.attn_grads_ref(q, k, v, up, c.H, scale, keep, p32)      # the SAME mask in forward and backward
    ref = dict(q=q, k=k, v=v, up=up, o=o, lse=lse, dq=dq, ck=ck, cv=cv, scale=scale)
    if c.N == 1:
        # one key: the softmax is constant, dq and dk are exactly zero (dS = P (dP - sum P dP) = dP - dP).  A relative
        # gate against zero means nothing; the error is measured against the term that cancels instead,
        # |scale * dP * K| for dq and scale * sum_q |dP * Q| for dk, with dP = dO . V per head
        hd = lambda x: x.double().view(c.B, -1, c.H, 32).transpose(1, 2)
        dp = (hd(up) * hd(v)).sum(-1, keepdim=True).abs()                                # (B, H, M, 1)
        ref["dq_scale"] = float((scale * dp * hd(k).abs()).max())
        ref["dk_scale"] = float((scale * (dp * hd(q).abs()).sum(2)).max())
        assert float(dq.abs().max()) < 1e-12 and float(ck[-1].abs().max()) < 1e-12
    return ref


def _call(lib, kv16, c, ref, blk):
    """One forward + backward at the C ABI on column block `blk`.  Returns every buffer the kernels could have
    written: views (o, lse, dq, dk_all, dv_all) and their guarded wholes."""
    B, H, M, N = c.B, c.H, c.M, c.N
    Cw = 32 * H
    W = 6 * Cw
    sdt = torch.bfloat16 if kv16 else torch.float32
    es = 2 if kv16 else 4
    k_all, _ = _sentinel(B * N, W, sdt)
    v_all, _ = _sentinel(B * N, W, sdt)
    k_all[:, blk * Cw:(blk + 1) * Cw] = ref["k"].reshape(B * N, Cw).to(sdt)
    v_all[:, blk * Cw:(blk + 1) * Cw] = ref["v"].reshape(B * N, Cw).to(sdt)
    if c.wide_q:
        qb, _ = _sentinel(B * M, 2 * Cw, torch.float32)
        qb[:, :Cw] = ref["q"].reshape(B * M, Cw)
        ldq = 2 * Cw
    else:
        qb, ldq = ref["q"].reshape(B * M, Cw), Cw
    o, o_w = _sentinel(B * M, Cw, torch.float32)
    lse, lse_w = _sentinel(B * H, M, torch.float32)
    dq, dq_w = _sentinel(B * M, Cw, torch.float32)
    dk_all, dk_w = _sentinel(B * N, W, sdt)
    dv_all, dv_w = _sentinel(B * N, W, sdt)
    off = es * blk * Cw
    fwd = lib.prh_attn_forward_kv16 if kv16 else lib.prh_attn_forward
    bwd = lib.prh_attn_backward_kv16 if kv16 else lib.prh_attn_backward
    assert fwd(_p(qb), ldq, _p(k_all, off), W, _p(v_all, off), W, _p(o), Cw, _p(lse), B, M, N, H, ref["scale"], c.p, SEED,
               0, _stream()) == 0
    assert bwd(_p(qb), ldq, _p(k_all, off), W, _p(v_all, off), W, _p(o), Cw, _p(lse), _p(ref["up"]), Cw, _p(dq), Cw,
               _p(dk_all, off), W, _p(dv_all, off), W, B, M, N, H, ref["scale"], c.p, SEED, 0, _stream()) == 0
    return dict(o=o, lse=lse, dq=dq, dk_all=dk_all, dv_all=dv_all, wholes=(o_w, lse_w, dq_w, dk_w, dv_w))


def _rel(x, ref):
    return float((x.double() - ref).norm() / (ref.norm() + 1e-300))


def _check(c, ref, out, blk, kv16):
    """All assertions on one call; returns {quantity: error / bound}."""
    B, H, M, N = c.B, c.H, c.M, c.N
    Cw = 32 * H
    r = {}
    r["o"] = float((out["o"].double() - ref["o"].reshape(B * M, Cw)).abs().max()) / GATE
    r["lse"] = float((out["lse"].double() - ref["lse"].reshape(B * H, M)).abs().max()) / GATE
    if N == 1:
        r["dq"] = float(out["dq"].double().abs().max()) / (GATE * ref["dq_scale"])
    else:
        r["dq"] = _rel(out["dq"], ref["dq"].reshape(B * M, Cw)) / GATE
    for name, buf, cum in (("dk", out["dk_all"], ref["ck"]), ("dv", out["dv_all"], ref["cv"])):
        got = buf[:, blk * Cw:(blk + 1) * Cw].double()
        cum = [t.reshape(B * N, Cw) for t in cum]
        zero_ref = N == 1 and name == "dk"
        if kv16:
            bound = R.bf16_store_bound(cum, GATE)
            if zero_ref:
                bound = bound + GATE * ref["dk_scale"]
            r[name] = float(((got - cum[-1]).abs() / bound).max())
            if len(cum) == 1:       # what ONE exact round-to-nearest of the reference itself uses of the bound
                r[name + "_rne"] = float(((cum[-1].float().to(torch.bfloat16).double() - cum[-1]).abs() / bound).max())
        elif zero_ref:
            r[name] = float(got.abs().max()) / (GATE * ref["dk_scale"])
        else:
            r[name] = _rel(got, cum[-1]) / GATE
        others = [i for i in range(6) if i != blk]
        assert _is_sentinel(buf.view(B * N, 6, Cw)[:, others]), f"{name}: a column block other than {blk} was written"
    for w, view_rows in zip(out["wholes"], (B * M, B * H, B * M, B * N, B * N)):
        assert _is_sentinel(w[:GUARD]) and _is_sentinel(w[GUARD + view_rows:]), "a guard row was written"
    for name, ratio in r.items():
        assert ratio < 1.0, f"{c.name} block {blk}: {name} error is {ratio:.3f} x its bound"      # NaN fails too
    return r


MARGINS = {}      # storage -> quantity -> largest error / bound seen in this process


@pytest.mark.parametrize("storage", list(STORAGES))
@pytest.mark.parametrize("case", CASES, ids=lambda c: c.name)
def test_attention_kernel_against_fp64(lib_mode, case, storage):
    """Gates: max |o - ref| < 2e-5, max |lse - ref| < 2e-5, rel-L2(dq) < 2e-5 (tests/test_attention_gpu.py's);
    dK / dV in fp32 storage rel-L2 < 2e-5, in bf16 storage elementwise
        |dk - c_last| <= 1.05 * 2^-8 * sum_t |c_t| + 2e-5 * max |c_last|
    (c_t: the reference's running sum after query tile t; the kernel rounds its running sum to bf16 once per tile).
    With one key (N = 1) dq and dk are exactly zero - the softmax is constant - and the relative gates are taken
    against the size of the terms that cancel instead (see _reference).
    Round-to-nearest reaches 2^-8 of the value itself just above a power of two, so with ~10^6 elements per case the
    bf16 ratio is expected near 1 / 1.05 = 0.95; dk_rne / dv_rne print what one exact rounding of the reference uses.
    Largest error / bound observed on an MI355X over all cases and column blocks: fp32 storage, mode 0: o 0.056,
    lse 0.057, dq 0.037, dk 0.024, dv 0.024; fp32 storage, mode 3: o 0.044, lse 0.044, dq 0.022, dk 0.021, dv 0.522
    (N = 1000; see the module docstring); bf16 storage, mode 4: o 0.044, lse 0.044, dq 0.022, dk 0.940 (one exact
    rounding: 0.940), dv 0.935 (0.935).
    """
    mode, kv16 = STORAGES[storage]
    lib = lib_mode(mode)
    ref = _reference(case)
    worst = MARGINS.setdefault(storage, {})
    for blk in BLOCKS:
        out = _call(lib, kv16, case, ref, blk)
        r = _check(case, ref, out, blk, kv16)
        for name, ratio in r.items():
            worst[name] = max(worst.get(name, 0.0), ratio)
        if case.twice and blk == BLOCKS[-1]:
            again = _call(lib, kv16, case, ref, blk)                # no atomics anywhere: the bits must repeat
            for name in ("o", "lse", "dq"):
                assert torch.equal(out[name], again[name]), f"{name} differs between two identical launches"
            for name in ("dk_all", "dv_all"):
                a, b = (t[name][:, blk * 32 * case.H:(blk + 1) * 32 * case.H] for t in (out, again))
                assert torch.equal(a, b), f"{name} differs between two identical launches"
    print(f"{case.name} {storage}: error / bound " + ", ".join(f"{k} {v:.3f}" for k, v in r.items()) +
          " | largest so far " + ", ".join(f"{k} {v:.3f}" for k, v in worst.items()))


def test_kv16_entries_refuse_what_they_cannot_run(lib_mode):
    """A leading dimension of K / V that is no multiple of 8 elements (the loader reads 16 bytes at a time), and the
    fp32 core of mode 0 (it has no bf16 load path): both return an error before anything is launched."""
    B, H, M, N = 2, 8, 32, 40
    Cw = 32 * H
    W = 6 * Cw
    g = torch.Generator().manual_seed(5)
    q = torch.randn(B * M, Cw, generator=g).cuda()
    up = torch.randn(B * M, Cw, generator=g).cuda()
    kv = torch.randn(B * N, W + 8, generator=g).to(torch.bfloat16).cuda()       # wide enough for the odd stride, too
    o_in = torch.randn(B * M, Cw, generator=g).cuda()
    lse_in = torch.randn(B * H, M, generator=g).cuda()

    def attempt(lib, ldk):
        o, o_w = _sentinel(B * M, Cw, torch.float32)
        lse, lse_w = _sentinel(B * H, M, torch.float32)
        dq, dq_w = _sentinel(B * M, Cw, torch.float32)
        dk, dk_w = _sentinel(B * N, W + 8, torch.bfloat16)
        dv, dv_w = _sentinel(B * N, W + 8, torch.bfloat16)
        rc_f = lib.prh_attn_forward_kv16(_p(q), Cw, _p(kv), ldk, _p(kv, 2 * Cw), ldk, _p(o), Cw, _p(lse), B, M, N, H,
                                         32.0 ** -0.5, 0.0, SEED, 0, _stream())
        rc_b = lib.prh_attn_backward_kv16(_p(q), Cw, _p(kv), ldk, _p(kv, 2 * Cw), ldk, _p(o_in), Cw, _p(lse_in), _p(up), Cw,
                                          _p(dq), Cw, _p(dk), ldk, _p(dv), ldk, B, M, N, H, 32.0 ** -0.5, 0.0, SEED, 0,
                                          _stream())
        torch.cuda.synchronize()
        assert rc_f != 0 and rc_b != 0
        assert lib.prh_last_error()
        for w in (o_w, lse_w, dq_w, dk_w, dv_w):
            assert _is_sentinel(w)

    attempt(lib_mode(4), W + 4)         # a multiple of 4, as the fp32 entries ask, but not of 8
    attempt(lib_mode(0), W)


def test_attention_arena_blocks_bf16_in_place_matches_out_of_place(lib_mode):
    """tests/test_attention_gpu.py::test_attention_arena_blocks_match_plain_path for bf16 storage: five attention_block
    calls on bf16 k_all / v_all in mode 4 (block 3 unused), once with the dK / dV blocks overwriting K / V
    (ops.KV_GRAD_IN_PLACE, the default) and once into buffers of their own.  The same kernels run on the same operands,
    so outputs, dq and the arena's dK_all / dV_all agree bit for bit unless a K / V tile is overwritten before its
    last read; the unused block is zero-filled."""
    from pointnet_refine_amd import ops
    lib_mode(4)
    B, M, N, H, Cw = 2, 32, 200, 8, 256
    g = torch.Generator().manual_seed(11)
    qs = [torch.randn(B, M, Cw, generator=g).cuda() for _ in range(6)]
    k_all = torch.randn(B, N, 6 * Cw, generator=g).to(torch.bfloat16).cuda()
    v_all = torch.randn(B, N, 6 * Cw, generator=g).to(torch.bfloat16).cuda()
    up = torch.randn(B, M, Cw, generator=g).cuda()
    used = (0, 1, 2, 4, 5)

    def run():
        q = [t.clone().requires_grad_(True) for t in qs]
        ka, va = k_all.clone().requires_grad_(True), v_all.clone().requires_grad_(True)
        token, arena = ops.kv_token(ka, va, Cw)
        outs = [ops.attention_block(q[i], ka, va, token, arena, i, H) for i in used]
        kept = [o.detach().clone() for o in outs]           # before the backward overwrites K / V in place
        sum((o * up).sum() for o in outs).backward()
        return kept, [q[i].grad.clone() for i in used], ka.grad.clone(), va.grad.clone()

    saved = ops.KV_GRAD_IN_PLACE
    try:
        ops.KV_GRAD_IN_PLACE = True
        o_a, dq_a, dk_a, dv_a = run()
        ops.KV_GRAD_IN_PLACE = False
        o_b, dq_b, dk_b, dv_b = run()
    finally:
        ops.KV_GRAD_IN_PLACE = saved
    assert dk_a.dtype == torch.bfloat16 and dk_a.shape == k_all.shape
    for a, b in zip(o_a + dq_a, o_b + dq_b):
        assert torch.equal(a, b)
    assert torch.equal(dk_a, dk_b) and torch.equal(dv_a, dv_b)
    assert torch.isfinite(dk_a.float()).all() and torch.isfinite(dv_a.float()).all()
    assert float(dk_a[..., 3 * Cw:4 * Cw].abs().max()) == 0.0 and float(dv_a[..., 3 * Cw:4 * Cw].abs().max()) == 0.0
    assert float(dk_a[..., :Cw].abs().max()) > 0.0 and float(dv_a[..., 5 * Cw:].abs().max()) > 0.0
    # and the values are those of the fp64 reference on the stored operands, to one bf16 rounding
    i = 5
    _, ck, cv = R.attn_grads_ref(qs[i], k_all[..., i * Cw:].contiguous(), v_all[..., i * Cw:].contiguous(), up, H, 32.0 ** -0.5)
    for got, cum in ((dk_a[..., i * Cw:], ck), (dv_a[..., i * Cw:], cv)):
        assert bool(((got.double() - cum[-1]).abs() <= R.bf16_store_bound(cum, GATE)).all())
