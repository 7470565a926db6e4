"""fp64 numpy restatement of the inference path of BASELINE config 5 (csrc/prh_attnfold.hpp): prh_posmem_images, the
two bf16 row images, and prh_attn_fold_forward, the cross-attention with the key / value projections folded in.  No
torch, no GPU.

Notation: bf16(.) is _stack_ref.bf16 (round to nearest even to 8 significant bits), fl32(.) one rounding to fp32.
"Stored order" is the image order of prh_cast_perm_bf16: position p of every group of 16 holds channel p with bits 2
and 3 swapped (perm_image; the map is its own inverse).

posmem_images_ref, per point r (rounded=True):
    h[k]   = max(fma(z, w0[k][2], fma(y, w0[k][1], fma(x, w0[k][0], b0[k]))), 0) in fp32 (each fma: an fp64
             multiply-add rounded once to fp32), a NULL b0 read as 0;  hb = bf16(h),  W2b = bf16(W2)
    pos[n] = sum_k W2b[n][k] hb[k]
    x16[r][n] = bf16((mem[r][n] + pos[n]) + b2[n]), a NULL b2 read as 0;  y16[r][n] = bf16(mem[r][n])
    both in stored order.

attn_fold_ref, per segment b, head h (32 channels), query q < M (rounded=True), X and Y the values the images hold,
un-permuted:
    qs    = bf16(fl32(q fl32(scale 1.4426950408889634f)));  Wkb = bf16(wk), Wvb = bf16(wv)
    Q'[c] = sum_{d<32} Wkb[32h+d][c] qs[32h+d];  Q'b = bf16(Q')
    S[key] = sum_c X[key][c] Q'b[c]                         (log2 units)
    keys in tiles of 32, in order: m_t = max(m_{t-1}, max_tile S), alpha = 2^(m_{t-1} - m_t), e = 2^(S - m_t),
        l <- l alpha + sum e (e unrounded),  PY[c] <- PY[c] alpha + sum_key bf16(e) Y[key][c];  keys >= N do not exist
    o[32h+d] = (sum_c Wvb[32h+d][c] bf16(PY[c])) (1/l) + bv[32h+d]
There is no key bias (constant along the keys: it drops out of the softmax).

rounded=False is the plain module arithmetic on the same operands: pos = relu(xyz W0^T + b0) W2^T + b2 with the two
images unrounded, and softmax(Q_h K_h^T scale) V_h with K = X Wk^T, V = Y Wv^T + bv.

accumulate=np.float32 evaluates the rounded chain once in fp32: every product is a float32 matmul, every elementwise
result passes through float32 in front of the same roundings, exp2 and the reciprocal are numpy's float32 ones.  It
exists to measure what one fp32 evaluation of the chain costs (tests/test_attnfold_ref_cpu.py); the gates of
tests/_attnfold_cases.py come from it and from nothing a kernel produced.

MUTATIONS names deliberate mistakes the reference can make on request (mutation=...): the faults of index arithmetic
the tests have to be able to see.
"""
import numpy as np

from _stack_ref import bf16

HEADS, HEAD_DIM, CH, TILE = 8, 32, 256, 32
LOG2E = 1.4426950408889634

# name: (the kernel it is a mistake of, what it does)
MUTATIONS = {
    "last_key_dropped": ("attn", "key N-1 is masked like the keys >= N"),
    "last_key_doubled": ("attn", "the last key of a partial tile counts twice"),
    "tail_unmasked": ("attn", "keys >= N of the last tile are not masked: the clamped copies of key N-1 count"),
    "no_swap": ("both", "bits 2 / 3 of the channel index are not swapped: image position p is taken for channel p"),
    "wv_next_head": ("attn", "head h multiplies by the Wv rows of head h+1"),
    "bv_next_head": ("attn", "head h adds the bv slice of head h+1"),
    "no_bv": ("attn", "bv is not added"),
    "scale_ignored": ("attn", "the softmax scale is 1/sqrt(32) whatever is passed"),
    "no_log2e": ("attn", "the scores are not converted to log2 units, and exp2 is still used"),
    "no_b2": ("posmem", "b2 is not added in x16"),
    "y_from_mempos": ("posmem", "y16 is the image of memory + pos"),
    "tile_skipped": ("posmem", "the first 256-point tile of the second grid-stride trip is never written"),
}


def _f64(a):
    return np.asarray(a, dtype=np.float64)


def _f32(a):
    return _f64(a).astype(np.float32).astype(np.float64)


_p = np.arange(16)
PERM = (np.arange(0, CH, 16)[:, None] + ((_p & 3) | ((_p & 4) << 1) | ((_p & 8) >> 1))[None, :]).reshape(CH)


def perm_image(rows):
    """[.., 256] values in channel order -> stored order."""
    return np.asarray(rows)[..., PERM]


def unperm_image(image):
    """Stored order -> channel order (swapping two bits is its own inverse)."""
    return np.asarray(image)[..., PERM]


def _mm(a, b, accumulate):
    if accumulate is np.float64:
        return np.matmul(_f64(a), _f64(b))
    return np.matmul(_f64(a).astype(np.float32), _f64(b).astype(np.float32)).astype(np.float64)


def posmem_images_ref(xyz, w0, b0, w2, b2, mem, rounded=True, accumulate=np.float64, mutation=None, grid=None,
                      details=False):
    """(x16, y16): the values of the two images, [P, 256] fp64 in stored order.  xyz [P, 3]; b0, b2 may be None.
    grid: the number of workgroups (tile_skipped only).  details: also a dict(h, pre, mag) - the hidden layer before
    its rounding, (mem + pos) + b2 before its rounding and |mem| + sum_k |W2b hb| + |b2|, in channel order."""
    assert mutation is None or MUTATIONS[mutation][0] in ("posmem", "both"), mutation
    r = _f32 if accumulate is np.float32 else _f64
    xyz, w0, w2, mem = _f64(xyz), _f64(w0), _f64(w2), _f64(mem)
    c0 = np.zeros(CH) if b0 is None else _f64(b0)
    c2 = np.zeros(CH) if b2 is None else _f64(b2)
    c2x = np.zeros(CH) if mutation == "no_b2" else c2
    if rounded:
        t = _f32(xyz[:, 0:1] * w0[None, :, 0] + c0[None, :])
        t = _f32(xyz[:, 1:2] * w0[None, :, 1] + t)
        h = np.maximum(_f32(xyz[:, 2:3] * w0[None, :, 2] + t), 0.0)
        hb, w2b = bf16(h), bf16(w2)
        pos = _mm(hb, w2b.T, accumulate)
        pre = r(r(mem + pos) + c2x[None, :])
        x, y = bf16(pre), bf16(r(mem + pos) if mutation == "y_from_mempos" else mem)
        mag = np.abs(mem) + np.abs(hb) @ np.abs(w2b).T + np.abs(c2)[None, :]
    else:
        h = np.maximum(xyz @ w0.T + c0[None, :], 0.0)
        pos = h @ w2.T
        pre = mem + pos + c2x[None, :]
        x, y = pre, (mem + pos if mutation == "y_from_mempos" else mem)
        mag = np.abs(mem) + np.abs(h) @ np.abs(w2).T + np.abs(c2)[None, :]
    if mutation != "no_swap":
        x, y = perm_image(x), perm_image(y)
    if mutation == "tile_skipped":
        x, y = x.copy(), y.copy()
        x[256 * grid:256 * grid + 256] = np.nan
        y[256 * grid:256 * grid + 256] = np.nan
    return (x, y, dict(h=h, pre=pre, mag=mag)) if details else (x, y)


def attn_fold_ref(q, X, Y, wk, wv, bv, B, M, N, scale, rounded=True, accumulate=np.float64, mutation=None,
                  details=False):
    """o [B*M, 256] fp64.  q [B*M, 256]; X, Y [B*N, 256] the values the images hold, in channel order; wk, wv
    [256, 256]; bv [256].  details: also a dict(S [B, H, M, N] scores in log2 units, l [B, H, M], PYb [B, H, M, 256]
    and mag [B*M, 256] = sum_c |Wvb bf16(PY)| (1/l) + |bv|)."""
    assert mutation is None or MUTATIONS[mutation][0] in ("attn", "both"), mutation
    f32 = accumulate is np.float32
    r = _f32 if f32 else _f64
    H, D = HEADS, HEAD_DIM
    q = _f64(q).reshape(B, M, H, D).transpose(0, 2, 1, 3)                  # [B, H, M, D]
    X, Y = _f64(X).reshape(B, N, CH), _f64(Y).reshape(B, N, CH)
    wk, wv, bv = _f64(wk).reshape(H, D, CH), _f64(wv).reshape(H, D, CH), _f64(bv).reshape(H, D)
    if mutation == "no_swap":
        X, Y = perm_image(X), perm_image(Y)
    if mutation == "scale_ignored":
        scale = 1.0 / np.sqrt(32.0)
    if mutation == "wv_next_head":
        wv = np.roll(wv, -1, axis=0)
    if mutation == "bv_next_head":
        bv = np.roll(bv, -1, axis=0)
    if mutation == "no_bv":
        bv = np.zeros_like(bv)
    if mutation == "last_key_dropped":
        X, Y = X[:, :N - 1], Y[:, :N - 1]
    extra = {"last_key_doubled": 1 if N % TILE else 0, "tail_unmasked": -N % TILE}.get(mutation, 0)
    if extra:
        X = np.concatenate([X, np.repeat(X[:, -1:], extra, axis=1)], axis=1)
        Y = np.concatenate([Y, np.repeat(Y[:, -1:], extra, axis=1)], axis=1)
    nk = X.shape[1]
    Xt = X.transpose(0, 2, 1)[:, None]                                     # [B, 1, 256, keys]
    if not rounded:
        K = np.matmul(Xt.transpose(0, 1, 3, 2), wk.transpose(0, 2, 1)[None])               # [B, H, keys, D]
        V = np.matmul(Y[:, None], wv.transpose(0, 2, 1)[None]) + bv[None, :, None, :]
        S = np.matmul(q, K.transpose(0, 1, 3, 2)) * scale
        P = np.exp(S - S.max(axis=-1, keepdims=True)) if nk else S
        P = P / P.sum(axis=-1, keepdims=True)
        o = np.matmul(P, V).transpose(0, 2, 1, 3).reshape(B * M, CH)
        return (o, dict(S=S * LOG2E)) if details else o
    c = np.float32(scale) * (np.float32(LOG2E) if mutation != "no_log2e" else np.float32(1.0))
    qs = bf16(_f32(q * float(c)))
    wkb, wvb = bf16(wk), bf16(wv)
    Qpb = bf16(_mm(qs, wkb[None], accumulate))                             # [B, H, M, 256]
    S = _mm(Qpb, Xt, accumulate)                                           # [B, H, M, keys]
    m = np.full((B, H, M), -np.inf)
    l = np.zeros((B, H, M))
    PY = np.zeros((B, H, M, CH))
    with np.errstate(invalid="ignore"):
        for k0 in range(0, nk, TILE):
            s = S[..., k0:k0 + TILE]
            m_new = np.maximum(m, s.max(axis=-1))
            if f32:
                alpha = np.exp2((m - m_new).astype(np.float32)).astype(np.float64)
                e = np.exp2((s - m_new[..., None]).astype(np.float32))
                l = _f32(l * alpha + e.sum(axis=-1, dtype=np.float32).astype(np.float64))
                e = e.astype(np.float64)
            else:
                alpha = np.exp2(m - m_new)
                e = np.exp2(s - m_new[..., None])
                l = l * alpha + e.sum(axis=-1)
            PY = r(r(PY * alpha[..., None]) + _mm(bf16(e), Y[:, None, k0:k0 + TILE], accumulate))
            m = m_new
        if nk == 0:
            l = l * np.nan                                                 # every key masked: 0 / 0 on the device
        PYb = bf16(PY)
        acc = _mm(PYb, wvb.transpose(0, 2, 1)[None], accumulate)           # [B, H, M, D]
        inv = r(1.0 / l)[..., None]
        o = r(acc * inv + bv[None, :, None, :])
    o = o.transpose(0, 2, 1, 3).reshape(B * M, CH)
    if not details:
        return o
    mag = np.matmul(np.abs(PYb), np.abs(wvb).transpose(0, 2, 1)[None]) * np.abs(inv) + np.abs(bv)[None, :, None, :]
    return o, dict(S=S, l=l, PYb=PYb, mag=mag.transpose(0, 2, 1, 3).reshape(B * M, CH))


# ------------------------------------------------------------------------------------------ bf16 bits and the x16 rule
def bits16(a):
    """The raw bf16 bits (uint16) of an array of bf16-representable values."""
    a = np.ascontiguousarray(a, np.float32)
    assert not (a.view(np.uint32) & 0xFFFF).any()
    return (a.view(np.uint32) >> 16).astype(np.uint16)


def from_bits16(h):
    return (np.ascontiguousarray(h).astype(np.uint32) << 16).view(np.float32).astype(np.float64)


def x16_rule(pre, mag, x, delta_rel):
    """The rule of the random posmem cases.  pre, mag: posmem_images_ref's details (fp64 accumulation), x: the values
    of an x16 image in channel order.  With delta = delta_rel * mag an element passes iff it is a bf16 value in
    [bf16(pre - delta), bf16(pre + delta)]: where no rounding boundary lies within delta of pre the two ends are
    bf16(pre) and the element must equal it bit for bit; where one does, it may be the neighbour on the other side of
    that boundary and nothing else.  (Where memory + pos + b2 cancels to less than 2^7 delta, more than one boundary
    lies within delta and the interval holds more than two values: one element in 10^5 of the Gaussian cases, and
    there a correct fp32 evaluation does differ by several ulps of its tiny result.)
    Returns (elements that break the rule, elements that differ from bf16(pre), elements within delta of a boundary,
    the smallest delta_rel that would admit every element)."""
    pre, x, ref = _f64(pre), _f64(x), bf16(pre)
    delta = delta_rel * _f64(mag)
    lo, hi = bf16(pre - delta), bf16(pre + delta)
    with np.errstate(invalid="ignore"):
        ok = (bf16(x) == x) & (x >= lo) & (x <= hi)
        half = np.ldexp(1.0, np.frexp(x)[1] - 9)                           # half a bf16 ulp of x (for the record only)
        need = np.where(x == ref, 0.0, np.maximum(np.abs(x - pre) - half, 0.0) / mag)
    return int((~ok).sum()), int((x != ref).sum()), int((lo != hi).sum()), float(np.max(need))
