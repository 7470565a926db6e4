"""The input sets of tests/test_mlp_stack_gpu.py, shared with tests/test_stack_ref_cpu.py: weights, x, dy and the fp64
reference of every case, plus the library's kernel-selection rules for the stack restated (csrc/prh_lib.hip:
nt_use_s3, tn_use_s3, tn_side_ok, dz_in_place, small_tn_dims_ok and the gemm_tn_direct condition of launch_tn)."""
from dataclasses import dataclass
from functools import lru_cache

import numpy as np

import _stack_ref as R

MOMENTUM, EPS = 0.25, 3e-5
POINT_MLP = (3, 64, 128, 256)
ENCODER = (4, 64, 128, 256, 512, 1024)
# The "gamma256" weights: seeded, with hidden layer 1's gamma x 2^8.  That divides dz of layer 2 by 2^8 and leaves dz of
# layer 1 as it was; with the plain seeded weights max|dz_1| / max|dz_2| is 3.6 to 4.4 at a last width of 256 and 5.3
# to 5.7 at 512, the smallest width at which the scaled pair is 2^10 apart
GAMMA_STACK, GAMMA_LAYER, GAMMA_FACTOR = (3, 64, 128, 512), 1, 2.0 ** 8


@dataclass(frozen=True)
class Case:
    widths: tuple
    P: int
    mode: int = 3
    training: int = 1
    relu_last: int = 0
    weights: str = "seeded"       # "point_mlp": procedural.linerefine_state_dict(0); "gamma256": seeded, one gamma x 2^8

    @property
    def name(self):
        w = "x".join(map(str, self.widths))
        return f"{self.weights}_{w}_P{self.P}_m{self.mode}_{'train' if self.training else 'eval'}_rl{self.relu_last}"

    @property
    def inputs(self):             # the key of the input set: cases that differ only in the mode share one reference
        return (self.widths, self.P, self.training, self.relu_last, self.weights)


def _pm(P, **kw):
    return Case(POINT_MLP, P, weights="point_mlp", **kw)


CASES = (
    [_pm(P) for P in (2, 77, 129, 513, 8000, 8192, 8197)] +
    [_pm(P, mode=m) for m in (0, 1, 4) for P in (77, 8197)] + [_pm(8192, mode=0)] +
    [_pm(P, training=t, relu_last=r) for P in (77, 8197) for t, r in ((1, 1), (0, 0), (0, 1))] +
    [Case(GAMMA_STACK, P, weights="gamma256") for P in (8192, 8197)] +
    [Case((6, 64, 128, 256, 512), 8197), Case(ENCODER, 8197), Case((64, 128, 64), 256), Case((64, 128, 64), 250),
     Case((64, 128, 64), 4160)])      # 4160: past gemm_tn_direct's 4096 rows, a multiple of 64: gemm_tn_small
BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES)


# ------------------------------------------------------------------------------------------ inputs
def _seeded_layers(widths, seed):
    g = np.random.default_rng([seed, len(widths)] + list(widths))
    layers, running = [], []
    for cin, cout in zip(widths[:-1], widths[1:]):
        layers.append(dict(w=(g.uniform(-1, 1, (cout, cin)) * 1.7 / np.sqrt(cin)).astype(np.float32),
                           b=g.uniform(-0.2, 0.2, cout).astype(np.float32),
                           gamma=g.uniform(0.5, 1.5, cout).astype(np.float32),
                           beta=g.uniform(-0.3, 0.3, cout).astype(np.float32)))
        running.append((g.uniform(-0.1, 0.1, cout).astype(np.float32), g.uniform(0.5, 1.5, cout).astype(np.float32)))
    return layers, running


def _point_mlp_layers():
    from oracle import procedural
    sd = procedural.linerefine_state_dict(0)
    layers, running = [], []
    for conv, bn in ((0, 1), (3, 4), (6, 7)):
        w = sd[f"point_mlp.{conv}.weight"]
        layers.append(dict(w=w.reshape(w.shape[0], -1).numpy().copy(), b=sd[f"point_mlp.{conv}.bias"].numpy().copy(),
                           gamma=sd[f"point_mlp.{bn}.weight"].numpy().copy(),
                           beta=sd[f"point_mlp.{bn}.bias"].numpy().copy()))
        running.append((sd[f"point_mlp.{bn}.running_mean"].numpy().copy(),
                        sd[f"point_mlp.{bn}.running_var"].numpy().copy()))
    return layers, running


@lru_cache(maxsize=None)
def inputs(key):
    """(layers, running, x, dy) of an input set, fp32 numpy, read-only.  x is uniform in +-25 (the +-25 m of the line
    encoder's coordinates) for the point_mlp weights and the 6-column stack, standard normal otherwise."""
    widths, P, training, relu_last, weights = key
    if weights == "point_mlp":
        layers, running = _point_mlp_layers()
        assert tuple([layers[0]["w"].shape[1]] + [ly["w"].shape[0] for ly in layers]) == widths
    else:
        layers, running = _seeded_layers(widths, 20240)
        if weights == "gamma256":
            layers[GAMMA_LAYER]["gamma"] = (layers[GAMMA_LAYER]["gamma"] * GAMMA_FACTOR).astype(np.float32)
    g = np.random.default_rng([7, P] + list(widths))
    if widths[0] in (3, 6):
        x = g.uniform(-25.0, 25.0, (P, widths[0])).astype(np.float32)
    else:
        x = g.standard_normal((P, widths[0])).astype(np.float32)
    dy = g.standard_normal((P, widths[-1])).astype(np.float32)
    for a in [x, dy] + [v for ly in layers for v in ly.values()] + [v for r in running for v in r]:
        a.setflags(write=False)
    return layers, running, x, dy


@lru_cache(maxsize=4)
def reference_forward(key):
    """The fp64 forward of an input set with the reference's own masks; computed once, shared, left unchanged."""
    widths, P, training, relu_last, weights = key
    layers, running, x, _ = inputs(key)
    return R.forward(x, layers, training, MOMENTUM, EPS, relu_last, running)


# ------------------------------------------------------------------------------------------ the library's rules
def cdiv(a, b):
    return -(-a // b)


def core_of(mode):                # stack_cores: mode 4 runs the stack on the split-fp16 cores
    return 3 if mode == 4 else mode


def nt_use_s3(core, M, N, K):
    return core != 0 and 64 <= K <= 4096 and N >= 128 and M >= 512 and cdiv(M, 256) * cdiv(N, 256) >= 32


def tn_use_s3(core, P, Mo, Ni):
    return core != 0 and Mo >= 128 and Ni >= 64 and P >= 8192


def dz_in_place(core, cols, ld):
    return core == 3 and cols % 4 == 0 and ld % 4 == 0


def tn_side_ok(core, P, Mo, Ni, ld, cols):
    # (the remaining conditions of the library's rule - at most 2048 workgroups, 16-B alignment - hold for every
    # stack here: a 256 x 256-tile plan of these widths has a few hundred workgroups)
    return core == 3 and ld <= 4096 and tn_use_s3(core, P, Mo, Ni) and (Mo | Ni | ld | cols) % 4 == 0 and cols <= 4096


def small_tn_dims_ok(P, Mo, Ni):
    return 64 <= P <= 16384 and P % 64 == 0 and Mo % 64 == 0 and Ni % 64 == 0


def tn_direct_ok(P, Mo, Ni):
    return 64 <= P <= 4096 and P % 64 == 0 and Mo % 32 == 0 and Ni % 32 == 0


def families(case):
    """Which kernel family serves each GEMM of the case: forward NT per layer, dgrad NT per layer (layer 0: dx), wgrad
    TN per layer ("+apply": held back, carrying the layer below's apply pass), and whether dz is materialised."""
    core, P, w = core_of(case.mode), case.P, case.widths
    L, ld = len(w) - 1, sum(w[1:])
    pad = lambda c: cdiv(c, 4) * 4
    gen = {0: None, 1: "s3", 3: "h2"}[core]
    mat = [dz_in_place(core, w[l + 1], ld) for l in range(L)]
    fwd, dgrad, wgrad = [], [], []
    for l in range(L):
        K, N = pad(w[l]), w[l + 1]
        fwd.append(gen if nt_use_s3(core, P, N, K) else "fp32")
        # dgrad of layer l: [P, cout] x [cout, cin]; the second generation needs a plain (materialised) operand
        split = nt_use_s3(core, P, w[l], N)      # layer 0 writes dx with N = cin0 unpadded
        dgrad.append(("h2" if mat[l] else "h2g1") if (split and core == 3) else (gen if split else "fp32"))
        Ni = pad(w[l])
        if tn_use_s3(core, P, N, Ni):
            fam = "h2tr" if (core == 3 and mat[l]) else ("h2g1" if core == 3 else "s3")
            if l > 0 and mat[l] and mat[l - 1] and tn_side_ok(core, P, N, Ni, ld, w[l]):
                fam += "+apply"
        elif l == 0 and mat[l] and tn_direct_ok(P, N, Ni):
            fam = "direct"
        elif l == 0 and mat[l] and small_tn_dims_ok(P, N, Ni):
            fam = "small"
        else:
            fam = "fp32"
        wgrad.append(fam)
    return dict(fwd=tuple(fwd), dgrad=tuple(dgrad), wgrad=tuple(wgrad), mat=all(mat))


# ------------------------------------------------------------------------------------------ gates
GATE_FWD = 2e-5       # max-abs / max(1, max|ref|): test_linear_with_fused_relu, test_attn_variants_gpu.GATE
GATE_GRAD = 1e-5      # rel-L2 per tensor: test_linear_fwd_bwd, the same GEMM cores


def fwd_ratio(ref, got):
    """Largest error as a multiple of the forward gate (<= 1 passes)."""
    ref, got = np.asarray(ref, np.float64), np.asarray(got, np.float64)
    return float(np.abs(ref - got).max() / (GATE_FWD * max(1.0, float(np.abs(ref).max()))))


def grad_ratio(ref, got):
    """rel-L2 error as a multiple of the gradient gate (<= 1 passes); an all-zero reference wants an all-zero result."""
    ref, got = np.asarray(ref, np.float64), np.asarray(got, np.float64)
    n = float(np.linalg.norm(ref))
    if n == 0.0:
        return 0.0 if not got.any() else float("inf")
    return float(np.linalg.norm(ref - got) / n / GATE_GRAD)


def db_ratio(ref_db, got_db, dz):
    """The bias gradient against sum|dz| of its columns: in training it is analytically zero, its own norm is noise."""
    scale = float(np.linalg.norm(np.abs(dz).sum(axis=0)))
    err = float(np.linalg.norm(np.asarray(ref_db, np.float64) - np.asarray(got_db, np.float64)))
    if scale == 0.0:
        return 0.0 if err == 0.0 else float("inf")
    return err / scale / GATE_GRAD


# P = 2 alone: BatchNorm's backward over two rows cancels to eps / (var + eps) of its terms (1e-6 and less here), and
# the kernels' dz = ca*dy + cb*z + cc takes its three coefficient vectors in fp32.  Rounding those vectors alone,
# everything else exact, costs rel-L2 1.6e-3 (dx), 1.4e-3 (dw) and 2.0e-3 of sum|dz| (db): that is arithmetic, shown
# on the CPU by test_two_rows_put_the_gradients_beyond_fp32_coefficients.  Measured on the MI355X: 2.14e-3, 7.0e-4,
# 1.64e-4; the gates are below four times those.  dgamma and dbeta, sums of dy, keep the common gate.
TWO_ROW_GATES = dict(dx=8e-3, dw=2.7e-3, db=6.4e-4)


def limits(P):
    """Largest error / GATE_GRAD allowed per backward quantity (1 everywhere but for dx, dw, db at P = 2)."""
    return {k: v / GATE_GRAD for k, v in TWO_ROW_GATES.items()} if P == 2 else {}
