"""numpy restatement of the second-stage reductions' order contract, and the
inputs that make an order visible.

Every output of these kernels is a fixed sequence of additions.  `chain` is the order inside one
chain (default `seq`: left to right from zero); `combine` is how the chains of one output are added
up.  test_ordered_reductions_cpu.py swaps other orders in to show that the inputs tell them apart;
test_ordered_reductions_gpu.py compares the kernels with the defaults, bit for bit.

Inputs: with plain Gaussian data a changed order almost never changes a float32 result, so each
summed column gets one +BIG / -BIG pair.  While the accumulator holds +-BIG every term added is
rounded away (BIG = 2^60 against fp64's 53 bits, 2^40 against fp32's 24), so the result is the sum of
exactly the terms that come before the first and after the second of the pair - a different set
under any other order."""
import numpy as np

BN_SLICES = 32
BIG64 = 2.0 ** 60
BIG32 = 2.0 ** 40


# ---------------------------------------------------------------- orders over axis 0
def seq(x):
    acc = np.zeros(x.shape[1:], x.dtype)
    for t in range(x.shape[0]):
        acc = acc + x[t]
    return acc


def reversed_order(x):
    return seq(x[::-1])


def pairwise(x):
    if x.shape[0] == 0:
        return np.zeros(x.shape[1:], x.dtype)
    while x.shape[0] > 1:
        h = x.shape[0] // 2
        y = x[0:2 * h:2] + x[1:2 * h:2]
        x = np.concatenate([y, x[2 * h:]], 0)
    return x[0]


def interleaved2(x):
    return seq(x[0::2]) + seq(x[1::2])


def ln_tree(c):
    return (c[0] + c[1]) + (c[2] + c[3])


def head_then_rest(c):
    """chain 0, then + chains 1..: the *_final kernels keep chain 0 in a register"""
    acc = c[0]
    for g in range(1, c.shape[0]):
        acc = acc + c[g]
    return acc


# ---------------------------------------------------------------- the kernels
def slabs(slab, chain=seq):
    """slab [S, len] float32 -> float32 [len]"""
    return chain(slab.astype(np.float64)).astype(np.float32)


def _slice_rows(R, sl):
    per = (R + BN_SLICES - 1) // BN_SLICES
    r0 = sl * per
    return r0, min(r0 + per, R)


def bn_stage1(ws_a, ws_b, N, tile_rows, P, forward, chain=seq, combine=seq):
    """ws_a / ws_b [R, ld] float32 -> [BN_SLICES, 3, N] float64"""
    R = ws_a.shape[0]
    out = np.zeros((BN_SLICES, 3, N), np.float64)
    a64, b64 = ws_a[:, :N].astype(np.float64), ws_b[:, :N].astype(np.float64)
    for sl in range(BN_SLICES):
        r0, r1 = _slice_rows(R, sl)
        rows = [np.arange(r0 + g, r1, 8) if r1 > r0 + g else np.zeros(0, np.int64) for g in range(8)]
        A = combine(np.stack([chain(a64[r]) for r in rows]))
        if not forward:
            out[sl, 0] = A
            out[sl, 1] = combine(np.stack([chain(b64[r]) for r in rows]))
            continue
        ni = [np.clip(P - r * tile_rows, 0, tile_rows).astype(np.float64) for r in rows]
        Nn = combine(np.stack([chain(np.broadcast_to(n[:, None], (len(n), N)).copy()) for n in ni]))
        mu = np.where(Nn > 0.0, A / np.where(Nn > 0.0, Nn, 1.0), 0.0)
        m2 = []
        for r, n in zip(rows, ni):
            keep = n > 0
            r, n = r[keep], n[keep][:, None]
            d = a64[r] / n - mu
            m2.append(chain(fma(d * d, np.broadcast_to(n, d.shape), b64[r])))
        out[sl, 0], out[sl, 1], out[sl, 2] = Nn, A, combine(np.stack(m2))
    return out


def fma(x, y, z):
    """x * y + z with one rounding, element-wise in float64: the compiler contracts the M2 term
    ws_b + d*d*ni into one fused multiply-add (as it did before the loads were batched).  y holds
    integers below 2^11, so the product is exact in the 64-bit mantissa of a long double; the sum is
    then rounded once to that mantissa and once to float64.  Where long double is no wider than
    float64 the product is split exactly (Veltkamp / Dekker) and added with an error-free sum."""
    if np.finfo(np.longdouble).nmant >= 63:
        p = x.astype(np.longdouble) * y.astype(np.longdouble)          # exact
        s = p + z.astype(np.longdouble)
        r = s.astype(np.float64)
        # double rounding: s sits exactly half-way between two float64 only if its low 11 bits are
        # 10000000000; resolve those with exact rational arithmetic
        low = (s - r.astype(np.longdouble))
        half = np.abs(low) == np.spacing(r).astype(np.longdouble) / 2
        if half.any():
            from fractions import Fraction
            for i in zip(*np.nonzero(half)):
                exact = Fraction(float(x[i])) * Fraction(float(y[i])) + Fraction(float(z[i]))
                r[i] = _round_fraction(exact)
        return r
    from fractions import Fraction
    r = np.empty(x.shape, np.float64)
    for i in np.ndindex(*x.shape):
        r[i] = _round_fraction(Fraction(float(x[i])) * Fraction(float(y[i])) + Fraction(float(z[i])))
    return r


def _round_fraction(q):
    return q.numerator / q.denominator          # int / int true division is correctly rounded


def partials(ws_a, ws_b, chain=seq, combine=seq):
    """ws_a, ws_b [R2, N] float32 (ws_b may be None: its output is 0) -> two float32 [N]"""
    def one(w):
        if w is None:
            return np.zeros(ws_a.shape[1], np.float32)
        w = w.astype(np.float64)
        return combine(np.stack([chain(w[g::32]) for g in range(32)])).astype(np.float32)
    return one(ws_a), one(ws_b)


def ln_param_grad(part_g, part_b, chain=seq, combine=ln_tree):
    def one(w):
        w = w.astype(np.float64)
        return combine(np.stack([chain(w[g::4]) for g in range(4)])).astype(np.float32)
    return one(part_g), one(part_b)


def partial_rows_final(part, chain=seq, combine=head_then_rest):
    """part [nblk, n_el] float32 -> float32 [n_el], all in float32"""
    assert part.dtype == np.float32
    return combine(np.stack([chain(part[g::16]) for g in range(16)]))


def pos_hidden_final(part, chain=seq, combine=head_then_rest):
    """part [nblk, 4 * H] -> dw0 [H, 3], db0 [H]"""
    s = partial_rows_final(part, chain, combine).reshape(-1, 4)
    return s[:, :3].copy(), s[:, 3].copy()


def act_amax(ws_c, ws_d, N, scale, shift):
    mx, mn = ws_c[:, :N].max(0), ws_d[:, :N].min(0)
    ok = mx >= mn
    v = np.maximum(_fmaf(mx, scale, shift), _fmaf(mn, scale, shift))
    return np.float32(max(0.0, float(v[ok].max()) if ok.any() else 0.0))


def _fmaf(x, y, z):
    # float32 fused multiply-add: the float64 product of two float32 is exact, and the float64 sum
    # is within 2^-53 relative - far from a float32 tie for the values the tests draw
    return (x.astype(np.float64) * y.astype(np.float64) + z.astype(np.float64)).astype(np.float32)


# ---------------------------------------------------------------- inputs
def with_pairs(rng, x, groups, big, across=False):
    """x [T, C] float32.  groups: list of row-index arrays, the chains of ONE output column set (all
    columns share them).  Writes one +big / -big pair per column: both in one random chain with at
    least two terms (across=False: the order inside a chain decides the result), or in two
    different chains (across=True: the order of the combine decides it).  Returns x."""
    C = x.shape[1]
    ok = [g for g in groups if len(g) >= (1 if across else 2)]
    if len(ok) < (2 if across else 1):
        return x
    lens = np.array([len(g) for g in ok])
    tab = np.zeros((len(ok), lens.max()), np.int64)
    for k, g in enumerate(ok):
        tab[k, :len(g)] = g
    cols = np.arange(C)
    g1 = rng.integers(len(ok), size=C)
    if across:       # a second, different chain; any term of each
        g2 = (g1 + 1 + rng.integers(len(ok) - 1, size=C)) % len(ok)
        i = (rng.random(C) * lens[g1]).astype(np.int64)
        j = (rng.random(C) * lens[g2]).astype(np.int64)
    else:            # two different terms of one chain
        g2 = g1
        i = (rng.random(C) * lens[g1]).astype(np.int64)
        j = (i + 1 + (rng.random(C) * (lens[g1] - 1)).astype(np.int64)) % lens[g1]
    x[tab[g1, i], cols] = big
    x[tab[g2, j], cols] = -big
    return x


def gauss(rng, *shape):
    return rng.standard_normal(shape).astype(np.float32)


def bn_groups(R):
    """chains of every slice: list over slices of 8 row-index arrays"""
    out = []
    for sl in range(BN_SLICES):
        r0, r1 = _slice_rows(R, sl)
        out.append([np.arange(r0 + g, r1, 8) if r1 > r0 + g else np.zeros(0, np.int64) for g in range(8)])
    return out


def strided_groups(T, J):
    return [np.arange(g, T, J) for g in range(J)]
