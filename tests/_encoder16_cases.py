"""The input sets of tests/test_encoder16_abi_gpu.py (prh_encoder_forward_bf16 / prh_encoder_backward_bf16 at the C ABI),
shared with tests/test_encoder16_ref_cpu.py, the launch rules of the two entry points restated (csrc/prh_lib.hip:
conv_in_fp32_ok, launch_nt_b16, tn_plan_b16, the combine kernel choice and the fuse_pool condition), and the gates of
the backward chain.

Weights, ctx, d_fused, d_gfeat, momentum, eps and the dead fusion channel are those of tests/_encoder_cases.py
(weights(C, od), inputs(key)); d_fused is handed over already rounded to bf16 (d_fused16).

Gates of the chained backward quantities.  The backward can only be compared as a chain (dy_f and dy_cat live in the
workspace), and along a chain of bf16 stores an fp32 evaluation differs from the fp64 one by more than fp32 arithmetic:
a result that lands on the other side of a bf16 rounding boundary moves by a whole bf16 ulp.  What that costs is
measured on the CPU from the reference alone (tests/test_encoder16_ref_cpu.py, test_the_gates_follow_from_what_one_
fp32_evaluation_costs): the store=bf16 chain of tests/_encoder_ref.py run twice on one saved forward, once in fp64 and
once with every GEMM and elementwise result (and the three BatchNorm-backward coefficient vectors) passed through
float32 in front of the same roundings.  FIGURES holds, per quantity, the largest error between the two over the
training input sets in the metric of _encoder_cases.quantities (rel-L2 per tensor; the training-mode db against
sum|dz|), rounded up; GATES = max(GATE_GRAD, 4 * figure) - 4 because numpy's summation order and the MFMA tile order
are different fp32 evaluations, and because flips are discrete events whose count varies at these sizes.  No figure
comes from a kernel's output.  Measured, largest over the seven training input sets (small, tails, c12, od512, mid,
mid_pool, od2048):
    layer    dw        dgamma    dbeta     db (of sum|dz|)
    fusion   3.58e-5   2.50e-5   2.74e-5   1.15e-8
    conv5    1.88e-4   1.31e-4   1.93e-4   9.38e-9
    conv4    7.09e-4   6.31e-4   7.16e-4   9.37e-9
    conv3    1.80e-3   1.73e-3   1.83e-3   1.16e-8
    conv2    3.14e-3   3.15e-3   3.46e-3   8.52e-9
    conv1    4.03e-3   4.41e-3   4.91e-3   6.22e-9
    d_ctx 3.87e-3   d_ctx[:, 3] 4.21e-3   d_gate_w1 1.12e-5   d_gate_b1 1.80e-5   d_gate_w2 1.24e-5   d_gate_b2 1.76e-5
These are not the 1e-5 to 1e-4 a single layer suggests.  One layer's stores flip at a rate of about 3e-5 per element
(an fp32 rounding of 6e-8 against a bf16 half-ulp of 2e-3) and each flip moves its element by 2^-8: rel-L2 near
3e-5, the fusion row.  But every dgrad below then starts from an operand that differs by that much EVERYWHERE, so a
share e / 2^-8 of its stores flip, and an error e becomes about sqrt(e * 2^-8): 3.6e-5, 1.9e-4, 7e-4, 1.8e-3, 3.1e-3,
4e-3 down the five convs - the chain runs into its fixed point, one bf16 ulp (3.9e-3).  Two correct fp32 evaluations
of conv1's gradients under this contract differ by a bf16 ulp; the gates say so, and are still 15 to 6000 times
tighter than the precision gates of tests/test_bf16_gpu.py.  tails (P = 35, 4760 elements per store) has no flip at
all: every figure of it is 4e-8 and below.  db in training is analytically zero and formed from the two sums, not from
the stored dz, so it sees no flip.  The eval-mode db is scale * dbeta and takes dbeta's gate (limits()).
"""
from dataclasses import dataclass
from functools import lru_cache

import numpy as np

import _encoder_cases as K
import _encoder_ref as E
import _stack_ref as S

MOMENTUM, EPS, DEAD, NBT0 = K.MOMENTUM, K.EPS, K.DEAD, K.NBT0
GATE_FWD, GATE_GRAD = K.GATE_FWD, K.GATE_GRAD
DG_ULPS = 8                       # band of the elementwise dG, in fp32 ulps of the product of magnitudes


@dataclass(frozen=True)
class Case:
    name: str
    C: int
    B: int
    N: int
    od: int = 1024
    training: int = 1
    pooled: int = 1               # gfeat and argmax requested from the forward
    d_fused: int = 1
    d_gfeat: int = 1
    d_ctx: int = 1

    @property
    def id(self):
        return f"{self.name}_{'train' if self.training else 'eval'}"

    @property
    def P(self):
        return self.B * self.N

    @property
    def cat(self):
        return sum(E.CONV_WIDTHS) + self.od

    @property
    def inputs(self):             # the key of _encoder_cases.inputs
        return (self.C, self.B, self.N, self.od, self.training)


CASES = (
    [Case("small", 4, 3, 43), Case("small", 4, 3, 43, training=0),
     Case("tails", 6, 5, 7, od=136, d_ctx=0), Case("tails", 6, 5, 7, od=136, d_ctx=0, training=0),
     Case("c12", 12, 3, 43, od=256), Case("od512", 4, 2, 128, od=512), Case("mid", 4, 3, 683),
     Case("mid_pool_gfeat_only", 4, 8, 256, d_fused=0),
     Case("mid_pool_fused_only", 4, 8, 256, pooled=0, d_gfeat=0),      # gfeat / argmax NULL: the path LineRefineNet takes
     Case("mid_pool_both", 4, 8, 256),
     # launch_nt_b16's LDS bound, 128 KB + 2 * (cdiv(K, 64) + 2) * 256 B <= 160 KB, accepts K = cat = 3008 (152.5 KB)
     Case("od2048", 4, 2, 128, od=2048)])
BY_ID = {c.id: c for c in CASES}
assert len(BY_ID) == len(CASES)
INPUT_SETS = sorted({c.inputs for c in CASES})
TRAINING_SETS = [k for k in INPUT_SETS if k[4]]


# ------------------------------------------------------------------------------------------ inputs
@lru_cache(maxsize=None)
def d_fused16(key):
    """d_fused of the input set as the bf16 buffer holds it, fp64, read-only."""
    a = S.bf16(K.inputs(key)[3])
    a.setflags(write=False)
    return a


def bits16(a):
    """The raw bf16 bits (uint16) of an array of bf16-representable values."""
    a = np.ascontiguousarray(a, np.float32)
    assert not (a.view(np.uint32) & 0xFFFF).any()
    return (a.view(np.uint32) >> 16).astype(np.uint16)


def from_bits16(h):
    return (np.ascontiguousarray(h).astype(np.uint32) << 16).view(np.float32).astype(np.float64)


@lru_cache(maxsize=None)
def saved_forward(key):
    """The store=bf16 forward of an input set in one fp32 evaluation, as a device would save it: z, scale, shift, mean
    and rstd are fp32-representable, the gate is the stored one.  Computed once, shared, left unchanged."""
    C, B, N, od, training = key
    prm, running, ctx, _, _ = K.inputs(key)
    return E.forward(ctx, B, N, prm, training, MOMENTUM, EPS, running, store=S.BF16_VIA_F32)


def chain(key, store, fw=None, d_fused=True, d_gfeat=True, mutation=None, masks=None):
    """The store=bf16 backward chain on a saved forward (default: saved_forward's, on its own masks)."""
    C, B, N, od, training = key
    prm, running, ctx, _, dg = K.inputs(key)
    fw = saved_forward(key) if fw is None else fw
    masks = E.own_masks(fw) if masks is None else masks
    return E.backward(d_fused16(key) if d_fused else None, dg if d_gfeat else None, ctx, B, N, prm, fw["conv"], fw["fus"],
                      training, masks, mutation=mutation, store=store, m_saved=fw["gate_stored"],
                      coeff_dtype=np.float32 if store.via is not None else None)


# ------------------------------------------------------------------------------------------ the library's rules
def cdiv(a, b):
    return -(-a // b)


def nt_b16_lds(K_, prologue):
    return 128 * 1024 + (2 * (cdiv(K_, 64) + 2) * 64 * 4 if prologue else 0)


def tn_plan_b16(P, Mo, Ni, maxld):
    """(splits, rows_per_split) of the bf16 wgrad."""
    tiles = cdiv(Mo, 256) * cdiv(Ni, 256)
    s = cdiv(768 if P >= 262144 else 256, tiles)
    best, bw = s, 1e9
    for c in range(s - 2 if s > 3 else 1, s + 5):
        w = cdiv(tiles * c, 256) * 256.0 / (tiles * c)
        if w < bw - 1e-3:
            bw, best = w, c
    s = max(1, min(best, max(1, cdiv(P, 512))))
    rps = max(32, cdiv(cdiv(P, s), 32) * 32)
    rps = min(rps, (2147483647 // (4 * max(maxld, 4))) // 32 * 32)
    return max(1, cdiv(P, rps)), rps


def families(case):
    """What serves each launch of the case.
    conv1: "valu" (conv_in_b16_kernel on fp32 operands) or "padded" (bf16 GEMM on rows padded to 8 channels);
    partial_k: the forward launches whose BN+ReLU prologue ends in a partial 64-deep k-tile; col_tail: the widths N
    that are no multiple of the 256-column tile; dgrad: per launch (fusion, conv5..2, gate) "dma" (gemm_nt_b16d_kernel,
    K % 64 == 0) or "staged" (gemm_nt_b16_kernel<PRO_NONE>); d_ctx: "staged_fp32" (launch_nt_b16<.., false>, K = 64)
    or None; combine: "scalar" or the threads per row of combine_bwd_b16v_kernel; pool: ("tiles", tiles per
    segment), ("kernel",) or None; row_tiles, stat_tiles (128 rows); splits: wgrad splits of fusion, conv5..2, gate
    (conv1 when padded); pacing: any wgrad with rows_per_split >= 16384 (scheduling only, out of scope)."""
    C, P, od, cat = case.C, case.P, case.od, case.cat
    w = (C,) + E.CONV_WIDTHS + (od,)
    c0p = cdiv(C, 8) * 8
    fwd_k = {f"conv{l + 1}": w[l] for l in range(1, 5)}
    fwd_k["fusion"] = cat
    dg_k = dict(fusion=od, conv5=od, conv4=512, conv3=256, conv2=128, gate=od)
    tn = dict(fusion=(od, cat, cat), conv5=(od, 512, cat), conv4=(512, 256, cat), conv3=(256, 128, cat),
              conv2=(128, 64, cat), gate=(od, 64, od))
    if C > 8:
        tn["conv1"] = (64, c0p, cat)
    plans = {k: tn_plan_b16(P, Mo, Ni, ld) for k, (Mo, Ni, ld) in tn.items()}
    return dict(conv1="valu" if C <= 8 else "padded",
                partial_k=tuple(k for k, v in fwd_k.items() if v % 64),
                col_tail=tuple(sorted({n for n in w[1:] + (cat,) if n % 256})),
                dgrad={k: "dma" if v % 64 == 0 else "staged" for k, v in dg_k.items()},
                d_ctx="staged_fp32" if case.d_ctx else None,
                combine=od // 8 if od in (256, 512, 1024, 2048) else "scalar",
                pool=None if not case.pooled else (("tiles", case.N // 128) if case.N % 128 == 0 else ("kernel",)),
                row_tiles=cdiv(P, 256), stat_tiles=cdiv(P, 128),
                splits={k: v[0] for k, v in plans.items()}, pacing=any(v[1] >= 16384 for v in plans.values()),
                lds_ok=nt_b16_lds(cat, True) <= 160 * 1024)


# ------------------------------------------------------------------------------------------ gates
quantities = K.quantities          # error / GATE_GRAD per backward quantity, from two results of _encoder_ref.backward

# quantity: (largest rel error of one fp32 evaluation of the store=bf16 chain against the fp64 one, the input set)
FIGURES = {
    "d_ctx": (4.0e-3, "small"), "d_ctx3": (4.3e-3, "small"),
    "conv1.dw": (4.2e-3, "od512"), "conv1.dgamma": (4.5e-3, "od512"), "conv1.dbeta": (5.1e-3, "od2048"),
    "conv1.db": (6.4e-9, "tails"),
    "conv2.dw": (3.3e-3, "small"), "conv2.dgamma": (3.3e-3, "od2048"), "conv2.dbeta": (3.6e-3, "small"),
    "conv2.db": (8.7e-9, "tails"),
    "conv3.dw": (1.9e-3, "od2048"), "conv3.dgamma": (1.8e-3, "small"), "conv3.dbeta": (1.9e-3, "od2048"),
    "conv3.db": (1.2e-8, "tails"),
    "conv4.dw": (7.3e-4, "od2048"), "conv4.dgamma": (6.5e-4, "od2048"), "conv4.dbeta": (7.3e-4, "od2048"),
    "conv4.db": (9.6e-9, "tails"),
    "conv5.dw": (2.0e-4, "mid"), "conv5.dgamma": (1.4e-4, "mid"), "conv5.dbeta": (2.0e-4, "od512"),
    "conv5.db": (9.6e-9, "tails"),
    "fusion.dw": (3.7e-5, "mid"), "fusion.dgamma": (2.6e-5, "mid"), "fusion.dbeta": (2.8e-5, "mid"),
    "fusion.db": (1.2e-8, "tails"),
    "d_gate_w1": (1.2e-5, "mid"), "d_gate_b1": (1.9e-5, "mid"), "d_gate_w2": (1.3e-5, "mid"), "d_gate_b2": (1.8e-5, "mid"),
}

GATES = {k: max(GATE_GRAD, 4.0 * v[0]) for k, v in FIGURES.items()}


def limits(training=1):
    """Largest error / GATE_GRAD allowed per backward quantity, the form _encoder_cases.quantities reports in.
    Eval mode: db is no longer analytically zero but scale * dbeta, column by column (dz = scale * dy), and is compared
    by rel-L2 like dbeta - it takes the gate of its layer's dbeta (tests/test_encoder16_ref_cpu.py measures it on the
    eval input sets: below the dbeta figure)."""
    lim = {k: v / GATE_GRAD for k, v in GATES.items()}
    if not training:
        lim.update({k: lim[k[:-2] + "dbeta"] for k in lim if k.endswith(".db")})
    return lim
