"""Numpy restatement of the BatchNorm-backward partial sums the gate backward writes, and inputs on which the
order of summation shows.

Contract (combine_bwd_kernel, and the recomputing epilogue EPI_GATE_BWD after it): ws_a / ws_b are
[ceil(P/64), C]; per 64-row block b and column there are four fp32 chains g = 0..3 over rows 64b + 16g + i,
i = 0..15 ascending, each doing s1 += dy and s2 = fma(dy, z, s2) from 0 and skipping rows >= P; the block's
value is ((c0 + c1) + c2) + c3.

Two other orders are restated for comparison: the lane-interleaved order of the vector epilogue's F_STATS sums
(a lane holds the rows r with r % 4 == rr, the four lane sums meet as (s0 + s1) + (s2 + s3)), and one plain
chain over the 64 rows.  All arithmetic is fp32, one rounding per step; s2 is restated for operands whose
product dy * z is exact in fp32 (z a power of two), where fma(dy, z, s) == fl(dy * z + s).
"""
import numpy as np

F = np.float32


def _chain(vals, acc=None):
    """Sequential fp32 sum of the rows of vals [n, C], starting from 0 (or acc)."""
    s = np.zeros(vals.shape[1], F) if acc is None else acc.astype(F)
    for v in vals:
        s = (s + v.astype(F)).astype(F)
    return s


def contract_partials(v):
    """v [P, C] fp32 -> [ceil(P/64), C]: four 16-row chains per block, ((c0 + c1) + c2) + c3."""
    P, C = v.shape
    nb = (P + 63) // 64
    out = np.zeros((nb, C), F)
    for b in range(nb):
        tot = None
        for g in range(4):
            lo = 64 * b + 16 * g
            c = _chain(v[lo:min(lo + 16, P)]) if lo < P else np.zeros(C, F)
            tot = c if tot is None else (tot + c).astype(F)
        out[b] = tot
    return out


def lane_interleaved_partials(v):
    """The F_STATS order on a 64-row block: lane sums over rows r % 4 == rr, then (s0 + s1) + (s2 + s3)."""
    P, C = v.shape
    nb = (P + 63) // 64
    out = np.zeros((nb, C), F)
    for b in range(nb):
        blk = v[64 * b:min(64 * b + 64, P)]
        s = [_chain(blk[rr::4]) for rr in range(4)]
        out[b] = ((s[0] + s[1]).astype(F) + (s[2] + s[3]).astype(F)).astype(F)
    return out


def plain_chain_partials(v):
    """One chain over the rows of each 64-row block."""
    P, C = v.shape
    nb = (P + 63) // 64
    return np.stack([_chain(v[64 * b:min(64 * b + 64, P)]) for b in range(nb)])


BIG = F(2.0 ** 24)


def cancelling_block():
    """[64, 4] fp32, one column per pattern; every pattern gives three different sums under the three orders.
    Column 0: +2^24 in chain 0, two ones at the head of chain 1, -2^24 at the head of chain 2
              (contract 2, lane-interleaved 1, plain chain 0).
    Column 1: the same one chain later (rows 16, 32, 33, 48).
    Column 2: the mirror image of column 0.
    Column 3: ones absorbed one at a time by a plain chain but kept by the 16-row chains."""
    v = np.zeros((64, 4), F)
    v[0, 0] = BIG; v[16, 0] = 1; v[17, 0] = 1; v[32, 0] = -BIG
    v[16, 1] = BIG; v[32, 1] = 1; v[33, 1] = 1; v[48, 1] = -BIG
    v[:, 2] = -v[:, 0]
    v[0, 3] = BIG; v[16:32, 3] = 1; v[33, 3] = 1; v[48, 3] = -BIG
    return v


def cancelling_matrix(P, C, seed=0):
    """[P, C] fp32: cancelling_block() tiled over every 64-row block and every group of 4 columns, each group
    scaled by a power of two, on top of small random values in the rows the patterns leave at zero."""
    rng = np.random.default_rng(seed)
    nb = (P + 63) // 64
    blk = cancelling_block()
    v = np.tile(blk, (nb, (C + 3) // 4))[:P, :C].copy()
    scale = np.exp2(rng.integers(-3, 4, size=(C + 3) // 4)).astype(F).repeat(4)[:C]
    v *= scale[None, :]
    fill = (rng.standard_normal((P, C)) * 0.25).astype(F)
    return np.where(v == 0, fill, v).astype(F)
