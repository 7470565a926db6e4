"""The input sets of tests/test_encoder_abi_gpu.py, shared with tests/test_encoder_ref_cpu.py: weights, ctx, d_fused,
d_gfeat and the fp64 reference forward of every case, plus the library's kernel-selection rules for the encoder
restated (csrc/prh_lib.hip: nt_use_s3, gate_on_h2, tn_use_s3, dz_in_place, the fuse_pool condition of
prh_encoder_forward and tn_side_ok for the held fusion wgrad; the stack's own rules come from tests/_stack_cases.py).

Weights: oracle.procedural.encoder_state_dict(C, out_dim, seed=3) with one fusion channel dead (fusion.1.weight[5] = 0,
fusion.1.bias[5] = -1, as tests/test_encoder_gpu.py): an all-zero column of `fused` whose arg-max must be point 0.
Every input set carries it - each is shared with at least one case that asks for the pooled output, and without the
pooling a dead channel is one more column.  ctx = procedural.synth_batch(B, N, C, 32, seed=11)[0]; d_fused and d_gfeat
are seeded standard normal; momentum = 0.25, eps = 3e-5 (tests/_stack_cases.py).
"""
from dataclasses import dataclass
from functools import lru_cache

import numpy as np

import _encoder_ref as E
import _stack_cases as SC

MOMENTUM, EPS = SC.MOMENTUM, SC.EPS
GATE_FWD, GATE_GRAD = SC.GATE_FWD, SC.GATE_GRAD
fwd_ratio, grad_ratio, db_ratio = SC.fwd_ratio, SC.grad_ratio, SC.db_ratio
DEAD = 5
NBT0 = 11                         # num_batches_tracked of layer l before the call: NBT0 + l


@dataclass(frozen=True)
class Case:
    name: str
    C: int
    B: int
    N: int
    od: int = 1024
    mode: int = 3
    training: int = 1
    pooled: int = 1               # gfeat and argmax requested from the forward
    d_fused: int = 1
    d_gfeat: int = 1
    recompute: int = 0            # forward gate = NULL, saved.gate_recompute = 1
    scratch: int = 0              # d_fused_scratch
    op_amax: int = 0

    @property
    def id(self):
        return f"{self.name}_m{self.mode}_{'train' if self.training else 'eval'}"

    @property
    def P(self):
        return self.B * self.N

    @property
    def inputs(self):             # the key of the input set: cases that differ in anything else share one reference
        return (self.C, self.B, self.N, self.od, self.training)


def _modes(modes, *a, **kw):
    return [Case(*a, mode=m, **kw) for m in modes]


_RECOMPUTE = dict(pooled=0, d_gfeat=0, recompute=1, scratch=1, op_amax=1)      # the path LineRefineNet takes
CASES = (
    _modes((0, 1, 3), "small", 4, 3, 43) +
    [Case("small_eval", 4, 3, 43, training=0)] +
    _modes((0, 3), "tails", 6, 5, 7, od=132) + _modes((0, 3), "tails", 6, 5, 7, od=132, training=0) +
    [Case("mid_recompute", 4, 3, 683, **_RECOMPUTE)] +
    _modes((0, 1, 3), "mid_stored", 4, 3, 683) +
    [Case("mid_pool", 4, 8, 256, d_fused=0), Case("mid_eval", 4, 3, 683, training=0),
     Case("big_recompute", 4, 7, 1171, **_RECOMPUTE)] +
    _modes((1, 3), "big_both", 4, 7, 1171) +
    [Case("big_c6", 6, 7, 1171, **_RECOMPUTE), Case("big_pool", 4, 16, 512)])
BY_ID = {c.id: c for c in CASES}
assert len(BY_ID) == len(CASES)
INPUT_SETS = sorted({c.inputs for c in CASES})


# ------------------------------------------------------------------------------------------ inputs
@lru_cache(maxsize=None)
def weights(C, od):
    """(prm, running) of _encoder_ref from the procedural state dict, fp32 numpy, read-only."""
    from oracle import procedural
    sd = procedural.encoder_state_dict(C, od, seed=3)
    sd["fusion.1.weight"][DEAD] = 0.0
    sd["fusion.1.bias"][DEAD] = -1.0
    n = lambda k: sd[k].float().reshape(sd[k].shape[0], -1).numpy().copy() if sd[k].dim() == 3 else sd[k].float().numpy().copy()
    layer = lambda conv, bn: dict(w=n(f"{conv}.weight"), b=n(f"{conv}.bias"), gamma=n(f"{bn}.weight"), beta=n(f"{bn}.bias"))
    names = [(f"conv{k}", f"bn{k}") for k in range(1, 6)] + [("fusion.0", "fusion.1")]
    prm = dict(conv=[layer(c, b) for c, b in names[:5]], fusion=layer(*names[5]),
               w1=n("intensity_gate.0.weight").reshape(-1), b1=n("intensity_gate.0.bias"),
               w2=n("intensity_gate.2.weight"), b2=n("intensity_gate.2.bias"))
    running = [(n(f"{b}.running_mean"), n(f"{b}.running_var")) for _, b in names]
    for a in [v for ly in prm["conv"] + [prm["fusion"]] for v in ly.values()] + \
            [prm[k] for k in ("w1", "b1", "w2", "b2")] + [v for r in running for v in r]:
        a.setflags(write=False)
    return prm, running


@lru_cache(maxsize=None)
def inputs(key):
    """(prm, running, ctx [P, C], d_fused [P, od], d_gfeat [B, 2*od]) of an input set, fp32 numpy, read-only."""
    from oracle import procedural
    C, B, N, od, training = key
    prm, running = weights(C, od)
    ctx = procedural.synth_batch(B, N, C, 32, seed=11)[0].numpy().reshape(B * N, C).copy()
    g = np.random.default_rng([13, B, N, C, od])
    d_fused = g.standard_normal((B * N, od)).astype(np.float32)
    d_gfeat = g.standard_normal((B, 2 * od)).astype(np.float32)
    for a in (ctx, d_fused, d_gfeat):
        a.setflags(write=False)
    return prm, running, ctx, d_fused, d_gfeat


@lru_cache(maxsize=2)
def reference_forward(key):
    """The fp64 forward of an input set on the reference's own masks; computed once, shared, left unchanged."""
    C, B, N, od, training = key
    prm, running, ctx, _, _ = inputs(key)
    return E.forward(ctx, B, N, prm, training, MOMENTUM, EPS, running)


# ------------------------------------------------------------------------------------------ the library's rules
def gate_on_h2(mode, P, od, C):
    return mode == 3 and SC.nt_use_s3(3, P, od, 64) and od % 4 == 0 and C <= 65536


def fuse_pool(case):
    return bool(case.pooled) and case.N % 128 == 0 and case.mode == 3 and SC.nt_use_s3(3, case.P, case.od, 64) and \
        case.od % 4 == 0


def fusion_held(core, P, od, cat):
    """The fusion wgrad waits for conv5's coefficients and carries conv5's apply pass: dz_f and dz_5 materialised
    and tn_side_ok (the side job is conv5's block of dy_cat, od columns of leading dimension cat)."""
    return SC.dz_in_place(core, od, od) and SC.dz_in_place(core, od, cat) and SC.tn_side_ok(core, P, od, cat, cat, od)


def families(case):
    """Which kernel family serves each launch of the case.  fwd: conv1..5, fusion, gate (NT); pool: "tiles" (F_POOL
    epilogue + pool_tiles_kernel), "kernel" (pool_kernel) or None; step1: "recompute" (EPI_GATE_BWD) or "combine"
    (combine_bwd_kernel); fusion: (wgrad, dgrad), "+apply": held back to carry conv5's apply pass; conv: the
    stack's families of tests/_stack_cases.py for the five convs (relu_last = 1)."""
    core, P, od, C = case.mode, case.P, case.od, case.C
    cat = sum(E.CONV_WIDTHS) + od
    gen = {0: None, 1: "s3", 3: "h2"}[core]
    pad = lambda c: SC.cdiv(c, 4) * 4
    w = (C,) + E.CONV_WIDTHS + (od,)
    nt = lambda M, N, K: gen if SC.nt_use_s3(core, M, N, K) else "fp32"
    fwd = tuple(nt(P, w[l + 1], pad(w[l])) for l in range(5)) + (nt(P, od, cat), nt(P, od, 64))
    matf = SC.dz_in_place(core, od, od)
    if SC.tn_use_s3(core, P, od, cat):
        wg = ("h2tr" if matf else "h2g1") if core == 3 else "s3"
        if core == 3 and fusion_held(core, P, od, cat):
            wg += "+apply"
    else:
        wg = "fp32"
    dg = nt(P, cat, od)
    if dg == "h2" and not matf:
        dg = "h2g1"
    # conv1..5 are the five-layer stack of tests/_stack_cases.py: its dy_cat has the leading dimension cat here too
    conv = SC.families(SC.Case(w, P, mode=core, training=case.training, relu_last=1))
    return dict(fwd=fwd, pool=None if not case.pooled else ("tiles" if fuse_pool(case) else "kernel"),
                step1="recompute" if case.recompute else "combine", recompute_ok=gate_on_h2(core, P, od, C),
                fusion=(wg, dg), conv_dgrad=conv["dgrad"], conv_wgrad=conv["wgrad"], mat=conv["mat"] and matf)


# ------------------------------------------------------------------------------------------ gates
def quantities(ref, got, training):
    """Error / gate of every backward quantity the GPU test compares (<= 1 passes there), from two results of
    _encoder_ref.backward."""
    q = dict(d_ctx=grad_ratio(ref["d_ctx"], got["d_ctx"]), d_ctx3=grad_ratio(ref["d_ctx"][:, 3], got["d_ctx"][:, 3]))
    for l, (a, b) in enumerate(zip(ref["conv"] + [ref["fusion"]], got["conv"] + [got["fusion"]])):
        name = f"conv{l + 1}" if l < 5 else "fusion"
        for k in ("dw", "dgamma", "dbeta"):
            q[f"{name}.{k}"] = grad_ratio(a[k], b[k])
        q[f"{name}.db"] = db_ratio(a["db"], b["db"], a["dz"]) if training else grad_ratio(a["db"], b["db"])
    for k in ("d_gate_w1", "d_gate_b1", "d_gate_w2", "d_gate_b2"):
        q[k] = grad_ratio(ref[k], got[k])
    return q


# The contract stores the gate m in fp32 and forms sig = 2m - 1 from it (gate_bwd_elem); where the sigmoid saturates
# 1 - sig cancels (pre-activations reach 12 on the largest inputs).  Rounding m ALONE to fp32 in the fp64 reference
# (tests/test_encoder_ref_cpu.py, test_what_the_fp32_stored_gate_costs) costs, as rel-L2, at most
#     d_gate_w2 1.4e-7   d_gate_b2 4.3e-8   d_gate_w1 1.3e-7   d_gate_b1 5.4e-8   d_ctx[:, 3] 2.6e-8
# over the small, tails, mid and big training input sets - a seventieth of the common gate of 1e-5 and less: dG =
# dF * r * 0.5*sig*(1-sig) is small exactly where its relative error is large.  No tensor has a gate of its own
# (rel-L2 per tensor name, were one ever needed: below four times such a CPU figure, never from a kernel's output).
OWN_GATES = {}
