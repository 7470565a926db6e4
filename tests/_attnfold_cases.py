"""The input sets of tests/test_attnfold_abi_gpu.py (prh_posmem_images / prh_attn_fold_forward at the C ABI), shared
with tests/test_attnfold_ref_cpu.py, and the gates of the random attention cases.

Five families.  Every attention case has 8 heads of 32 channels; X and Y are generated as bf16 values (what the images
hold), so the device receives exactly the reference's operands.

onehot    B = 2, M in {32, 7}, N in {1, 31, 32, 33, 64, 65, 97, 129}.  Wk is a dense orthogonal matrix, every key has a
          random +-1 code of 32 bits per head and X = bf16(codes Wk), so that the projected key X Wk_h^T is the key's code
          of head h up to rounding; the query of (b, h, q) is 512 times the code of its winner.  The winner's score then
          exceeds every other key's by 2 * 512 * scale * log2(e) = 261 log2 units per differing code bit.  The builder
          asserts a margin >= 160 on the rounded reference for every (b, h, q): 2^-160 is zero in fp32, so P is exactly
          one-hot and l exactly 1 whichever tile the winner sits in, and  o = Wvb_h Y[winner] + bv_h.  Winners cover key 0,
          key N-1 and both sides of every 32-key boundary, and differ between heads and between queries.
uniform   B = 2, N in {1, 31, 33, 65, 85}, q = 0: every score is 0, l = N exactly, Y holds integers in {1, 2, 3} so that
          every column sum is an integer <= 255, exact in bf16, and  o = Wvb_h (sum_key Y) / N + bv_h.  A dropped, doubled
          or unmasked key changes an integer.
random    Gaussian inputs, (B, M, N) in {(2, 32, 64), (2, 20, 33), (3, 32, 200), (1, 7, 1)}, scale 1/sqrt(32) and 0.25 on
          (3, 32, 200); (2, 20, 33) has strided operands: q a slice of a packed [.., 768] buffer, ldwk = ldwv = ldo = 260.
posmem_exact   small integers throughout: xyz in {-1, 0, 1}, w0 in {-1, 0, 1}, b0 in {-1, 0} (h in {0..3}), w2 in
          {-1, 0, 1} with 8 non-zeros per row, b2 in [-8, 8], mem in [-100, 100]: every intermediate is an integer below
          256 and both images are known bit for bit.  Rows {1, 31, 33, 255, 257, 777} and 256 * CUs + 33 (the workgroups
          are persistent, grid = min(tiles, CUs): only then does one take a second trip), ldx in {3, 4, 6}, ldm in
          {256, 260}; every case runs with all four combinations of NULL / given b0 and b2.
posmem_random  Gaussian inputs (pos at a tenth of memory: see X16_DELTA below), rows {100, 777}, both biases given.

Gates.  The exact attention families have a derived elementwise gate, EXACT_GATE * mag with mag = sum_c |Wvb PYb| (1/l)
+ |bv|: a 256-deep fp32 accumulation plus two roundings is bounded by 258 * 2^-24 ~ 2^-16 of the absolute sum, and 4x
covers the matrix instruction's internal order and the reciprocal.  The posmem families are compared bit for bit
(posmem_random's x16 under the rule of _attnfold_ref.x16_rule).  The gates of the random attention cases are MEASURED,
on the CPU, from the reference alone (tests/test_attnfold_ref_cpu.py::test_the_gates_follow_from_what_one_fp32_
evaluation_costs): the rounded chain evaluated once in fp32 against the same chain in fp64 - what one fp32 evaluation
costs, bf16 roundings that flip because of it included.  FIGURES holds, per case, that rel-L2 and the largest
|delta| / max|ref|; GATES = 4 * the largest figure over the cases: the matrix instructions sum in another order than
numpy, and the hardware's exp2 and reciprocal are good to 1 ulp.  No figure comes from a kernel's output.
"""
from dataclasses import dataclass
from functools import lru_cache

import numpy as np

import _attnfold_ref as R
from _stack_ref import bf16

H, D, CH = R.HEADS, R.HEAD_DIM, R.CH
SCALE = 1.0 / np.sqrt(32.0)
EXACT_GATE = 2.0 ** -14           # of mag, elementwise: the exact attention families
MARGIN = 160.0                    # log2 units; 2^-160 is zero in fp32
QMAG = 512.0
# The x16 rule of the random posmem cases (_attnfold_ref.x16_rule): an element may sit on the other side of a bf16
# rounding boundary only where the reference's pre-rounding value is within X16_DELTA * mag of that boundary, mag = |mem|
# + sum_k |W2b hb| + |b2|; such elements must be fewer than X16_SHARE of all.  The first reading of this rule had 2^-15
# (twice the worst case 258 * 2^-24 of one 256-deep fp32 sum and two additions).  That cannot go with the 1 % limit: a
# band of 2 delta around one boundary per ulp, ulp <= 2^-7 |pre|, exempts a share 2^-14 mag / ulp >= 2^-7 m of the
# elements (m in [1, 2) the mantissa of pre), 1.1 % on average even when mag = |pre|, and 20 % measured on unit-scale
# Gaussian inputs, where mag is 8 |pre| at the median.  Kept: the 1 % limit.  Tightened: delta, to 2^-18 - the worst case
# of the kernel's own order of summation, 16 chained matrix instructions of 16 products each with at most three
# roundings per instruction, plus the two additions: 50 * 2^-24 < 2^-18.  (One fp32 evaluation on the CPU stays within
# 2^-23 mag.)  Whatever passes at 2^-18 passes at 2^-15.  The Gaussian cases keep pos at a tenth of memory (w0, b0 ~
# N(0, 1) / 4; w2, b2 ~ N(0, 1) / 64: pos ~ 0.09 rms, still 10 to 20 bf16 ulps of memory), which puts 0.75 % of the
# elements inside delta.
X16_DELTA = 2.0 ** -18
X16_SHARE = 0.01


@dataclass(frozen=True)
class AttnCase:
    family: str
    B: int
    M: int
    N: int
    scale: float = SCALE
    ldq: int = 256
    ldw: int = 256                # ldwk = ldwv
    ldo: int = 256

    @property
    def id(self):
        s = "" if self.scale == SCALE else f"_scale{self.scale}"
        return f"{self.family}_B{self.B}_M{self.M}_N{self.N}{s}{'_strided' if self.ldo != 256 else ''}"

    @property
    def seed(self):
        return 1000 * self.N + 10 * self.M + self.B


ONEHOT = [AttnCase("onehot", 2, M, N) for N in (1, 31, 32, 33, 64, 65, 97, 129) for M in (32, 7)]          # B, M, N above
UNIFORM = [AttnCase("uniform", 2, M, N) for N, M in ((1, 32), (31, 7), (33, 32), (65, 7), (85, 32))]
RANDOM = [AttnCase("random", 2, 32, 64), AttnCase("random", 2, 20, 33, ldq=768, ldw=260, ldo=260),
          AttnCase("random", 3, 32, 200, scale=0.25), AttnCase("random", 1, 7, 1)]
ATTN_CASES = ONEHOT + UNIFORM + RANDOM


def special_keys(N):
    """Key 0, key N-1 and both sides of every 32-key boundary."""
    return sorted({0, N - 1} | {k for t in range(32, N, 32) for k in (t - 1, t)})


@lru_cache(maxsize=None)
def attn_inputs(case):
    """dict(q [B*M, 256], X, Y [B*N, 256] (bf16 values, channel order), wk, wv [256, 256], bv [256]) as float32, read-only;
    the exact families add winners [B, H, M] (onehot), expect and mag [B*M, 256] (the closed form and its absolute sum)."""
    B, M, N = case.B, case.M, case.N
    g = np.random.default_rng(case.seed)
    d = dict(wv=g.standard_normal((CH, CH)) / 16, bv=g.standard_normal(CH))
    if case.family == "onehot":
        d["wk"] = np.linalg.qr(g.standard_normal((CH, CH)))[0]
        codes = g.choice([-1.0, 1.0], size=(B, N, CH))
        d["X"] = bf16(codes @ d["wk"]).reshape(B * N, CH)                  # X Wk^T = codes (Wk Wk^T = 1)
        d["Y"] = bf16(g.standard_normal((B * N, CH)))
        pool = special_keys(N)
        pool = pool + [k for k in g.permutation(N).tolist() if k not in pool][:13 - len(pool)]     # 13 keys, or all N
        bI, hI, mI = np.arange(B)[:, None, None], np.arange(H)[None, :, None], np.arange(M)[None, None, :]
        win = np.asarray(pool)[(mI + 3 * hI + 5 * bI) % len(pool)]         # [B, H, M]
        d["winners"] = win
        qh = codes.reshape(B, N, H, D)[bI, win, hI]                        # [B, H, M, D]: head h's slice of the winner's code
        d["q"] = (QMAG * qh).transpose(0, 2, 1, 3).reshape(B * M, CH)
    else:
        d["wk"] = g.standard_normal((CH, CH)) / 16
        d["X"] = bf16(g.standard_normal((B * N, CH)))
        if case.family == "uniform":
            d["Y"] = g.integers(1, 4, size=(B * N, CH)).astype(np.float64)
            d["q"] = np.zeros((B * M, CH))
        else:
            d["Y"] = bf16(g.standard_normal((B * N, CH)))
            d["q"] = g.standard_normal((B * M, CH))
    d = {k: (v if k == "winners" else np.asarray(v, np.float64).astype(np.float32)) for k, v in d.items()}
    if case.family in ("onehot", "uniform"):
        wvb = bf16(d["wv"]).reshape(H, D, CH)
        Yb = d["Y"].astype(np.float64).reshape(B, N, CH)
        if case.family == "onehot":
            PYb, inv = Yb[np.arange(B)[:, None, None], d["winners"]], 1.0                  # [B, H, M, 256]
        else:
            PYb, inv = np.broadcast_to(Yb.sum(axis=1)[:, None, None, :], (B, H, M, CH)), 1.0 / N
        bvh = d["bv"].astype(np.float64).reshape(1, H, 1, D)
        flat = lambda a: a.transpose(0, 2, 1, 3).reshape(B * M, CH)
        d["expect"] = flat(np.matmul(PYb, wvb.transpose(0, 2, 1)[None]) * inv + bvh)
        d["mag"] = flat(np.matmul(np.abs(PYb), np.abs(wvb).transpose(0, 2, 1)[None]) * inv + np.abs(bvh))
        check_exact_preconditions(case, d)
    for v in d.values():
        v.setflags(write=False)
    return d


def margins(case, d, S):
    """Winner's score minus the best other key's, [B, H, M] (inf where N = 1), from the reference's scores."""
    w = d["winners"][..., None]
    top = np.take_along_axis(S, w, axis=-1)[..., 0]
    rest = S.copy()
    np.put_along_axis(rest, w, -np.inf, axis=-1)
    return top - rest.max(axis=-1)


def check_exact_preconditions(case, d):
    """What makes the closed forms exact, asserted on the rounded reference for every (b, h, q) - none is skipped."""
    B, M, N = case.B, case.M, case.N
    _, det = R.attn_fold_ref(d["q"], d["X"], d["Y"], d["wk"], d["wv"], d["bv"], B, M, N, case.scale, details=True)
    if case.family == "onehot":
        mg = margins(case, d, det["S"])
        assert mg.shape == (B, H, M) and (mg >= MARGIN).all(), (case.id, float(mg.min()))
        win = d["winners"]
        assert set(special_keys(N)) <= set(win.reshape(-1).tolist()), case.id
        if N > 1:
            assert all(len(set(win[b, :, m].tolist())) > 1 for b in range(B) for m in range(M)), case.id      # between heads
            assert all(len(set(win[b, h].tolist())) > 1 for b in range(B) for h in range(H)), case.id         # between queries
    else:
        sums = d["Y"].astype(np.float64).reshape(B, N, CH).sum(axis=1)
        assert (det["S"] == 0).all() and (det["l"] == N).all(), case.id
        assert (sums == np.rint(sums)).all() and sums.max() <= 255 and (bf16(sums) == sums).all(), case.id


def attn_reference(case, **kw):
    d = attn_inputs(case)
    return R.attn_fold_ref(d["q"], d["X"], d["Y"], d["wk"], d["wv"], d["bv"], case.B, case.M, case.N, case.scale, **kw)


@lru_cache(maxsize=None)
def random_reference(case):
    """(o, details) of a random case: rounded, fp64 accumulation.  Computed once, shared, left unchanged."""
    o, det = attn_reference(case, details=True)
    o.setflags(write=False)
    return o, det


def errors(ref, got):
    """(rel-L2, largest |delta| / max|ref|) - the two figures of the random attention cases."""
    ref, got = np.asarray(ref, np.float64), np.asarray(got, np.float64)
    if not np.isfinite(got).all():
        return float("inf"), float("inf")
    return (float(np.linalg.norm(got - ref) / np.linalg.norm(ref)), float(np.abs(got - ref).max() / np.abs(ref).max()))


# case id: (rel-L2, largest |delta| / max|ref|) of the rounded chain in one fp32 evaluation against the fp64 one, rounded up
FIGURES = {
    "random_B2_M32_N64": (1.4e-5, 1.8e-4),
    "random_B2_M20_N33_strided": (3.1e-5, 3.3e-4),
    "random_B3_M32_N200_scale0.25": (1.8e-5, 1.6e-4),
    "random_B1_M7_N1": (4.8e-8, 5.4e-8),           # one key: no softmax, no flip - fp32 arithmetic alone
}
GATES = dict(rel_l2=4.0 * max(v[0] for v in FIGURES.values()), max_rel=4.0 * max(v[1] for v in FIGURES.values()))


# ------------------------------------------------------------------------------------------ posmem
@dataclass(frozen=True)
class PosmemCase:
    family: str
    rows: int                     # 0: 256 * CUs + 33, known on the device only
    ldx: int
    ldm: int

    @property
    def id(self):
        return f"{self.family}_rows{self.rows if self.rows else '256cu+33'}_ldx{self.ldx}_ldm{self.ldm}"

    def resolved(self, cus):
        return self if self.rows else PosmemCase(self.family, 256 * cus + 33, self.ldx, self.ldm)


POSMEM_EXACT = [PosmemCase("posmem_exact", r, ldx, ldm)            # rows, ldx, ldm
                for r, ldx, ldm in ((1, 3, 256), (31, 4, 260), (33, 6, 256), (255, 3, 260), (257, 4, 256), (777, 6, 260),
                                    (0, 4, 260))]
POSMEM_RANDOM = [PosmemCase("posmem_random", 100, 4, 256), PosmemCase("posmem_random", 777, 3, 260)]
BIAS_COMBOS = [(b0, b2) for b0 in (False, True) for b2 in (False, True)]
CPU_CUS = 2                       # the stand-in for the CU count where there is no device: 545 rows, 3 tiles, 2 workgroups


@lru_cache(maxsize=4)
def posmem_inputs(case):
    """dict(xyz [rows, 3], w0 [256, 3], b0, w2 [256, 256], b2, mem [rows, 256]) as float32, read-only."""
    assert case.rows > 0
    g = np.random.default_rng(7 * case.rows + case.ldx)
    P = case.rows
    if case.family == "posmem_exact":
        w2 = np.zeros((CH, CH))
        cols = np.argsort(g.random((CH, CH)), axis=1)[:, :8]
        np.put_along_axis(w2, cols, g.choice([-1.0, 1.0], size=(CH, 8)), axis=1)
        d = dict(xyz=g.integers(-1, 2, size=(P, 3)), w0=g.integers(-1, 2, size=(CH, 3)), b0=g.integers(-1, 1, size=CH),
                 w2=w2, b2=g.integers(-8, 9, size=CH), mem=g.integers(-100, 101, size=(P, CH)))
    else:
        d = dict(xyz=g.standard_normal((P, 3)), w0=g.standard_normal((CH, 3)) / 4, b0=g.standard_normal(CH) / 4,
                 w2=g.standard_normal((CH, CH)) / 64, b2=g.standard_normal(CH) / 64, mem=g.standard_normal((P, CH)))
    d = {k: np.asarray(v, np.float32) for k, v in d.items()}
    for v in d.values():
        v.setflags(write=False)
    return d


def posmem_exact_expected(d):
    """Yields (b0_on, b2_on, x, y) for the four bias combinations of an exact case: the two images in channel order,
    float32, by integer arithmetic alone (every product and sum below is exact in float32), with the preconditions
    asserted: h in {0..3}, every intermediate an integer below 256."""
    assert (np.count_nonzero(d["w2"], axis=1) == 8).all()
    for b0_on in (False, True):
        h = np.maximum(d["xyz"] @ d["w0"].T + (d["b0"] if b0_on else np.float32(0)), np.float32(0))
        pos = h @ d["w2"].T
        s = d["mem"] + pos
        assert h.min() >= 0 and h.max() <= 3
        for b2_on in (False, True):
            x = s + d["b2"] if b2_on else s
            for a in (h, pos, s, x, d["mem"]):
                assert (a == np.rint(a)).all() and np.abs(a).max() < 256
            yield b0_on, b2_on, x, d["mem"]


def posmem_reference(case, b0_on=True, b2_on=True, **kw):
    d = posmem_inputs(case)
    return R.posmem_images_ref(d["xyz"], d["w0"], d["b0"] if b0_on else None, d["w2"], d["b2"] if b2_on else None,
                               d["mem"], **kw)


# ------------------------------------------------------------------------------------------ teeth
FAMILIES = dict(onehot="attn", uniform="attn", random="attn", posmem_exact="posmem", posmem_random="posmem")

# (family, mutation): why the mutation cannot move the family's compared quantity, by construction
CANNOT_BITE = {
    ("onehot", "last_key_doubled"): "a winner counted twice doubles PY and l alike: Wvb (2 Y[w]) / 2",
    ("onehot", "tail_unmasked"): "copies of key N-1 either lose by the margin or multiply PY and l alike",
    ("onehot", "scale_ignored"): "the cases use 1/sqrt(32), and any positive scale keeps the winner",
    ("onehot", "no_log2e"): "the margin of 160 log2 units is still 110 without the factor: P stays one-hot",
    ("uniform", "scale_ignored"): "q = 0: every score is 0 at any scale",
    ("uniform", "no_log2e"): "q = 0: every score is 0 in any unit",
}


def applies(family, mutation):
    kernel = R.MUTATIONS[mutation][0]
    return kernel in (FAMILIES[family], "both")
