"""prh_posmem_images / prh_attn_fold_forward / prh_cast_perm_bf16 (the inference path of BASELINE config 5) at the C ABI
against tests/_attnfold_ref.py, the fp64 restatement of csrc/prh_attnfold.hpp with every rounding in its place.  This is
the "kernels compute what they say" check; tests/test_attnfold_gpu.py answers the other question, whether bf16 operands
are good enough (2e-2 / 5e-2 against the unrounded module).

Attention, exact families (tests/_attnfold_cases.py: onehot, uniform): the closed forms o = Wvb_h Y[winner] + bv_h and
o = Wvb_h (sum Y) / N + bv_h, elementwise |o - ref| <= 2^-14 mag with mag = sum_c |Wvb PYb| (1/l) + |bv| - derived: a
256-deep fp32 accumulation plus two roundings is within 258 * 2^-24 ~ 2^-16 of the absolute sum, and 4 x covers the
matrix instruction's internal order and the reciprocal.  Attention, random family: rel-L2 and largest |delta| /
max|ref| against the rounded reference, with the gates measured on the CPU from the reference alone (GATES = 4 x what
one fp32 evaluation of the chain costs: rel_l2 1.24e-4, max_rel 1.32e-3).  Every o has one extra row and, where
ldo = 260, four extra columns, prefilled with NaN: those stay NaN, every row < B*M is finite.

posmem, exact family: both images bit-equal to integer arithmetic, with every combination of NULL / given b0 and b2,
ldx in {3, 4, 6}, ldm in {256, 260}, and 256 * CUs + 33 rows, where the persistent workgroups take a second trip.  The
unused columns of xyz and memory hold NaN.  posmem, random family: y16 bit-equal; x16 bit-equal except where the
reference's pre-rounding value lies within 2^-18 (|mem| + sum|W2b hb| + |b2|) of a bf16 rounding boundary, where it may
land on the other side (_attnfold_ref.x16_rule; a condition on every element, not a share).  The images have one extra
row of bf16 NaN bits, which stays.

Argument contract: H = 4, M = 33, N = 0, a leading dimension of 258 and a NULL operand are refused with nothing
written; rows = 0 returns 0 with nothing written.  prh_posmem_images used to accept any ldm >= 256 although its memory
rows are read with 16-byte loads; it now refuses ldm % 4 != 0 as prh_cast_perm_bf16 does.  The test asserts the
refusal only - no misaligned call was ever launched.

Observed on an MI355X (every test prints its own):
    onehot   largest |o - ref| / gate 0.0011 over the 16 cases;  uniform 0.0007 over the 5
    random   rel_l2 / gate, max_rel / gate:  B2_M32_N64 0.124 0.162 | B2_M20_N33_strided 0.000 0.000 (no rounding
             flipped) | B3_M32_N200_scale0.25 0.126 0.101 | B1_M7_N1 0.001 0.000
    posmem_exact   no differing bit in either image, any bias combination, 1 to 65569 rows (257 tiles on 256 workgroups)
    posmem_random  y16 bit-equal; x16: 0 of 25600 and 1 of 198912 elements differ, the one 2^-25.4 mag from its boundary
No finding: the kernels compute what csrc/prh_attnfold.hpp says, and the statement of the arithmetic needed no correction.
"""
import ctypes as C

import numpy as np
import pytest
import torch

import _attnfold_cases as K
import _attnfold_ref as R

pytestmark = pytest.mark.gpu

BF16_NAN = 0x7FC0


def _lib():
    from pointnet_refine_amd import _lib as L
    return L.lib()


def _p(t, offset=0):
    return C.c_void_p(0 if t is None else t.data_ptr() + offset)


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _padded(a, ld, col0=0):
    """a [rows, w] inside a NaN [rows, ld] buffer at column col0; returns (buffer, byte offset of a[0, 0])."""
    a = torch.from_numpy(np.array(a, np.float32))
    buf = torch.full((a.shape[0], ld), float("nan"))
    buf[:, col0:col0 + a.shape[1]] = a
    return buf.cuda(), 4 * col0


def _image(values):
    """bf16 values in channel order -> the device image (int16 bits, stored order)."""
    return torch.from_numpy(R.bits16(R.perm_image(values)).view(np.int16)).cuda()


def _nan_image(rows):
    return torch.full((rows + 1, 256), BF16_NAN, dtype=torch.int16, device="cuda")


def _bits(t):
    return t.cpu().numpy().view(np.uint16)


class Attn:
    """Device copies of an attention case and the entry point around them."""

    def __init__(self, case):
        d = K.attn_inputs(case)
        self.case, self.rows = case, case.B * case.M
        self.q, self.qoff = _padded(d["q"], case.ldq, 256 if case.ldq >= 768 else 0)      # a slice of a packed q|k|v buffer
        self.x16, self.y16 = _image(d["X"]), _image(d["Y"])
        self.wk, _ = _padded(d["wk"], case.ldw)
        self.wv, _ = _padded(d["wv"], case.ldw)
        self.bv = torch.from_numpy(np.array(d["bv"])).cuda()
        self.o = torch.full((self.rows + 1, case.ldo), float("nan"), device="cuda")

    def __call__(self, null=(), **over):
        c = self.case
        a = dict(ldq=c.ldq, ldwk=c.ldw, ldwv=c.ldw, ldo=c.ldo, B=c.B, M=c.M, N=c.N, H=8, scale=c.scale)
        a.update(over)
        t = {k: None if k in null else getattr(self, k) for k in ("q", "x16", "y16", "wk", "wv", "bv", "o")}
        rc = _lib().prh_attn_fold_forward(_p(t["q"], self.qoff if t["q"] is not None else 0), a["ldq"], _p(t["x16"]), _p(t["y16"]),
                                          _p(t["wk"]), a["ldwk"], _p(t["wv"]), a["ldwv"], _p(t["bv"]), _p(t["o"]), a["ldo"],
                                          a["B"], a["M"], a["N"], a["H"], a["scale"], 0, _stream())
        torch.cuda.synchronize()
        return rc

    def output(self):
        """o [B*M, 256] as fp64, after the checks every case shares: rows < B*M finite, the rest still NaN."""
        o = self.o.cpu().numpy().astype(np.float64)
        assert np.isfinite(o[:self.rows, :256]).all()
        assert np.isnan(o[self.rows]).all() and np.isnan(o[:, 256:]).all()
        return o[:self.rows, :256]

    def untouched(self):
        return bool(torch.isnan(self.o).all())


# ------------------------------------------------------------------------------------------ attention
EXACT = K.ONEHOT + K.UNIFORM


@pytest.mark.parametrize("case", EXACT, ids=[c.id for c in EXACT])
def test_exact_attention_cases(case):
    d = K.attn_inputs(case)
    at = Attn(case)
    assert at() == 0, _lib().prh_last_error()
    o = at.output()
    ratio = np.abs(o - d["expect"]) / (K.EXACT_GATE * d["mag"])
    print(f"ATTNFOLD {case.id} largest |o - ref| / gate = {ratio.max():.4f}")
    assert (ratio <= 1.0).all(), (case.id, float(ratio.max()), int((ratio > 1).sum()))


@pytest.mark.parametrize("case", K.RANDOM, ids=[c.id for c in K.RANDOM])
def test_random_attention_cases_against_the_rounded_reference(case):
    ref, _ = K.random_reference(case)
    at = Attn(case)
    assert at() == 0, _lib().prh_last_error()
    rel, mx = K.errors(ref, at.output())
    print(f"ATTNFOLD {case.id} rel_l2 = {rel:.3e} ({rel / K.GATES['rel_l2']:.3f} of its gate)  "
          f"max_rel = {mx:.3e} ({mx / K.GATES['max_rel']:.3f} of its gate)")
    assert rel <= K.GATES["rel_l2"] and mx <= K.GATES["max_rel"], (case.id, rel, mx, K.GATES)


# ------------------------------------------------------------------------------------------ posmem
class Posmem:
    def __init__(self, case, d):
        self.rows = case.rows
        self.xyz, _ = _padded(d["xyz"], case.ldx)
        self.mem, _ = _padded(d["mem"], case.ldm)
        self.ldx, self.ldm = case.ldx, case.ldm
        dev = lambda a: torch.from_numpy(np.array(a)).cuda()
        self.w0, self.b0, self.w2, self.b2 = dev(d["w0"]), dev(d["b0"]), dev(d["w2"]), dev(d["b2"])
        self.x16, self.y16 = _nan_image(self.rows), _nan_image(self.rows)

    def __call__(self, null=(), **over):
        a = dict(ldx=self.ldx, ldm=self.ldm, rows=self.rows)
        a.update(over)
        t = {k: None if k in null else getattr(self, k) for k in ("xyz", "w0", "b0", "w2", "b2", "mem", "x16", "y16")}
        rc = _lib().prh_posmem_images(_p(t["xyz"]), a["ldx"], _p(t["w0"]), _p(t["b0"]), _p(t["w2"]), _p(t["b2"]), _p(t["mem"]),
                                      a["ldm"], a["rows"], _p(t["x16"]), _p(t["y16"]), 0, _stream())
        torch.cuda.synchronize()
        return rc

    def images(self):
        """(x16, y16) bits [rows, 256] after the check that the extra row still holds its NaN bits."""
        x, y = _bits(self.x16), _bits(self.y16)
        assert (x[self.rows] == BF16_NAN).all() and (y[self.rows] == BF16_NAN).all()
        return x[:self.rows], y[:self.rows]

    def reset(self):
        self.x16.fill_(BF16_NAN)
        self.y16.fill_(BF16_NAN)

    def untouched(self):
        return bool((self.x16 == BF16_NAN).all()) and bool((self.y16 == BF16_NAN).all())


@pytest.mark.parametrize("case", K.POSMEM_EXACT, ids=[c.id for c in K.POSMEM_EXACT])
def test_exact_posmem_cases_bit_for_bit(case):
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    case = case.resolved(cus)
    d = K.posmem_inputs(case)
    pm = Posmem(case, d)
    for b0_on, b2_on, x, y in K.posmem_exact_expected(d):
        pm.reset()
        null = (() if b0_on else ("b0",)) + (() if b2_on else ("b2",))
        assert pm(null=null) == 0, _lib().prh_last_error()
        gx, gy = pm.images()
        wx, wy = R.bits16(R.perm_image(x)), R.bits16(R.perm_image(y))
        bad = int((gx != wx).sum()), int((gy != wy).sum())
        print(f"POSMEM {case.id} rows={case.rows} tiles={-(-case.rows // 256)} workgroups={min(-(-case.rows // 256), cus)} "
              f"b0={b0_on} b2={b2_on} differing x16 / y16 = {bad}")
        assert bad == (0, 0), (case.id, b0_on, b2_on, bad, np.argwhere(gx != wx)[:4].tolist(), np.argwhere(gy != wy)[:4].tolist())


@pytest.mark.parametrize("case", K.POSMEM_RANDOM, ids=[c.id for c in K.POSMEM_RANDOM])
def test_random_posmem_cases_under_the_x16_rule(case):
    d = K.posmem_inputs(case)
    x, y, det = K.posmem_reference(case, details=True)
    pm = Posmem(case, d)
    assert pm() == 0, _lib().prh_last_error()
    gx, gy = pm.images()
    assert np.array_equal(gy, R.bits16(y))
    got = R.unperm_image(R.from_bits16(gx))
    bad, differ, inside, need = R.x16_rule(det["pre"], det["mag"], got, K.X16_DELTA)
    print(f"POSMEM {case.id} x16: {differ} of {got.size} differ from the reference, {inside} within delta of a boundary, "
          f"{bad} break the rule; delta needed 2^{np.log2(need) if need else -np.inf:.1f} of mag (allowed 2^-18)")
    assert bad == 0


# ------------------------------------------------------------------------------------------ argument contract
SMALL = K.RANDOM[0]                # B 2, M 32, N 64, every leading dimension 256
PM_SMALL = K.POSMEM_EXACT[2]       # 33 rows, ldx 6, ldm 256


def _wide(case, **kw):
    """The case with room for a leading dimension of up to 260 in every buffer (the refused calls launch nothing, and
    would stay in bounds if they did)."""
    return K.AttnCase(case.family, case.B, case.M, case.N, case.scale, **kw)


def test_attention_refuses_what_it_was_not_built_for():
    at = Attn(SMALL)
    for over in (dict(H=4), dict(M=33), dict(N=0), dict(B=0), dict(M=0)):
        assert at(**over) != 0, over
        assert at.untouched(), over
    for k in ("q", "x16", "y16", "wk", "wv", "bv", "o"):
        assert at(null=(k,)) != 0, k
        assert at.untouched(), k
    wide = Attn(_wide(SMALL, ldq=260, ldw=260, ldo=260))
    for k in ("ldq", "ldo", "ldwk", "ldwv"):
        assert wide(**{k: 258}) != 0, k
        assert b"multiples of 4" in _lib().prh_last_error()
        assert wide.untouched(), k
    assert wide() == 0 and at() == 0                                        # and the same buffers are accepted as they are
    assert np.array_equal(wide.output(), at.output())


def test_posmem_refuses_bad_arguments_and_a_memory_stride_its_loads_cannot_take():
    d = K.posmem_inputs(PM_SMALL)
    pm = Posmem(K.PosmemCase(PM_SMALL.family, PM_SMALL.rows, 6, 260), d)
    for over in (dict(ldm=258), dict(ldm=257), dict(ldm=259), dict(ldm=252), dict(ldx=2), dict(rows=-1)):
        assert pm(**over) != 0, over
        assert pm.untouched(), over
    for k in ("xyz", "w0", "w2", "mem", "x16", "y16"):
        assert pm(null=(k,)) != 0, k
        assert pm.untouched(), k
    assert pm(rows=0) == 0 and pm.untouched()
    assert pm() == 0 and not pm.untouched()


def test_cast_perm_refuses_a_stride_of_258_and_accepts_no_rows():
    src = torch.randn(4, 260, device="cuda")
    dst = _nan_image(4)
    call = lambda s, ld, t, rows: _lib().prh_cast_perm_bf16(_p(s), ld, _p(t), rows, 0, _stream())
    for args in ((src, 258, dst, 4), (src, 252, dst, 4), (None, 260, dst, 4), (src, 260, None, 4), (src, 260, dst, -1)):
        assert call(*args) != 0
    assert call(src, 260, dst, 0) == 0
    torch.cuda.synchronize()
    assert bool((dst == BF16_NAN).all())
    assert call(src, 260, dst, 4) == 0
    torch.cuda.synchronize()
    assert np.array_equal(_bits(dst)[:4], R.bits16(R.perm_image(src[:, :256].to(torch.bfloat16).float().cpu().numpy())))
    assert (_bits(dst)[4] == BF16_NAN).all()
