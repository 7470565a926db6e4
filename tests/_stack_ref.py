"""fp64 numpy reference of a shared-MLP stack: L layers of Linear + BatchNorm1d (+ ReLU), forward and backward.

A layer is a dict(w [cout, cin], b, gamma, beta); `running` is a list of (running_mean, running_var).  Every array is
taken to fp64 on entry.  Layer l is followed by a ReLU when l < L - 1 or relu_last is set.  The ReLU is written as
where(mask, y, 0) so that masks taken elsewhere - from the device's own z, scale and shift (device_masks) - can stand
in for the layer's own y > 0: with the masks fixed the stack is Linear + BatchNorm only, and two evaluations differ by
arithmetic error alone.  No torch, no GPU.

`store` is the one storage hook of both passes.  None is the fp32 contract: nothing is rounded and every statement
below is the plain fp64 one.  A Store (BF16, BF16_VIA_F32) is the bf16-storage contract of the *_bf16 entry points: it
is applied wherever that contract stores or feeds a 16-bit value, and to nothing else -
    forward   A = store(relu(z_prev * scale + shift)) and W = store(W) feed every GEMM (the first layer's x and W too
              unless store_first = 0: the VALU first layer on fp32 operands), z = store(A W^T + b), and the BatchNorm
              statistics are those of the stored z;
    backward  dz = store(ca*dy + cb*z + cc) (db stays the sum of the unrounded expression: bn_bwd_finalize_kernel
              forms it from the partial sums), dw = dz^T A with the stored dz and the stored A of the forward,
              dx = dz store(W), and a masked dx that a buffer holds (l > 0) is stored.
"""
import numpy as np

MUTATIONS = ("no_constant_term", "biased_running_var", "relu_last_ignored", "dgrad_unmasked")


def _f64(a):
    return np.asarray(a, dtype=np.float64)


def bf16(a):
    """Round to nearest even to 8 significant bits (v_cvt_pk_bf16_f32; the exponent range is fp32's and is not
    modelled: no value here comes near it)."""
    m, e = np.frexp(_f64(a))
    return np.ldexp(np.rint(m * 256.0), e - 8)


class Store:
    """store(a): the value a 16-bit buffer or operand holds for the result a.  `via`: a type every result passes
    through first (np.float32: one fp32 evaluation of the contract, as a kernel's fp32 registers; None: fp64)."""

    def __init__(self, rounding=bf16, via=None):
        self.rounding, self.via = rounding, via

    def result(self, a):
        return _f64(a) if self.via is None else _f64(_f64(a).astype(self.via))

    def __call__(self, a):
        return self.rounding(self.result(a))


BF16, BF16_VIA_F32 = Store(), Store(via=np.float32)


def stored(store, a):
    """What a 16-bit buffer or operand holds (a itself in the fp32 contract)."""
    return a if store is None else store(a)


def result(store, a):
    """A result that stays in fp32 (accumulators, statistics, parameter gradients)."""
    return a if store is None else store.result(a)


def has_relu(l, L, relu_last):
    return l < L - 1 or bool(relu_last)


def batchnorm(z, ly, rn, training, momentum, eps, mutation=None, store=None):
    """mean, rstd, scale, shift and the running statistics after the call, of the z given (with a store: the stored z)."""
    gamma, beta = _f64(ly["gamma"]), _f64(ly["beta"])
    rm, rv = _f64(rn[0]), _f64(rn[1])
    P = z.shape[0]
    if training:
        mean = result(store, z.mean(axis=0))
        m2 = ((z - mean) ** 2).sum(axis=0)
        rstd = result(store, 1.0 / np.sqrt(m2 / P + eps))
        new_rm = (1.0 - momentum) * rm + momentum * mean
        new_rv = (1.0 - momentum) * rv + momentum * (m2 / (P if mutation == "biased_running_var" else P - 1))
    else:
        mean, rstd, new_rm, new_rv = rm, 1.0 / np.sqrt(rv + eps), rm, rv
    scale = result(store, gamma * rstd)
    shift = result(store, beta - mean * scale)
    return dict(mean=mean, rstd=rstd, scale=scale, shift=shift, running_mean=new_rm, running_var=new_rv)


def forward(x, layers, training, momentum, eps, relu_last, running, masks=None, mutation=None, store=None,
            store_first=1):
    """Per layer: z, mean, rstd (biased variance), scale, shift, y (post-BN), running_mean / running_var after the call
    (unbiased variance, as nn.BatchNorm1d; unchanged in eval), mask (the layer's own y > 0) and out.
    mutation: one of MUTATIONS, a deliberate mistake (tests/test_stack_ref_cpu.py shows the inputs detect each)."""
    L = len(layers)
    h = _f64(x)
    recs = []
    for l, ly in enumerate(layers):
        w, b = _f64(ly["w"]), _f64(ly["b"])
        if l > 0 or store_first:
            h, w = stored(store, h), stored(store, w)
        z = stored(store, h @ w.T + b)
        bn = batchnorm(z, ly, running[l], training, momentum, eps, mutation, store)
        y = z * bn["scale"] + bn["shift"]
        own = y > 0
        if has_relu(l, L, relu_last):
            out = np.where(own if masks is None else masks[l], y, 0.0)
        else:
            out = y
        recs.append(dict(z=z, y=y, mask=own, out=out, **bn))
        h = out
    return recs


def records_from_saved(z_cat, scale, shift, mean, rstd, widths, relu_last, masks):
    """The records backward() reads, rebuilt from what a forward call saved (z_cat and the concatenated coefficient
    vectors) and the given masks: the backward of a saved forward, whoever ran it."""
    L = len(widths)
    off = np.concatenate([[0], np.cumsum(widths)])
    recs = []
    for l in range(L):
        s = slice(off[l], off[l + 1])
        z, sc, sh = _f64(z_cat[:, s]), _f64(scale[s]), _f64(shift[s])
        y = z * sc + sh
        out = np.where(masks[l], y, 0.0) if has_relu(l, L, relu_last) else y
        recs.append(dict(z=z, mean=_f64(mean[s]), rstd=_f64(rstd[s]), scale=sc, shift=sh, y=y, out=out))
    return recs


def backward(dy, x, layers, recs, training, relu_last, masks, mutation=None, coeff_dtype=None, store=None,
             store_first=1, dy_stats=None):
    """dx and, per layer, dw, db, dgamma, dbeta (and dz, for the tests' scales) from the records of a forward.
    Training: the full BatchNorm backward.  Eval: dz = scale * dy.
    coeff_dtype: round the three BatchNorm-backward coefficient vectors to this type and nothing else - what storing
    them in fp32 alone costs (at P = 2 the terms of dz cancel to eps / (var + eps) of themselves).
    store, store_first: the storage hook (module docstring).  dy_stats: what the last layer's two BatchNorm sums are
    taken from when not from dy itself (a deliberate mistake of tests/_encoder_ref.py)."""
    L = len(layers)
    P = recs[0]["z"].shape[0]
    g = _f64(dy)
    if relu_last and mutation != "relu_last_ignored":
        g = np.where(masks[L - 1], g, 0.0)
    grads = [None] * L
    for l in range(L - 1, -1, -1):
        r = recs[l]
        w, gamma = _f64(layers[l]["w"]), _f64(layers[l]["gamma"])
        xhat = (r["z"] - r["mean"]) * r["rstd"]
        gs = g if dy_stats is None or l < L - 1 else _f64(dy_stats)
        dbeta = result(store, gs.sum(axis=0))
        dgamma = result(store, (gs * xhat).sum(axis=0))
        if training:
            dz = gamma * r["rstd"] * (g - dbeta / P - xhat * (dgamma / P))
            if coeff_dtype is not None:
                # the same dz in the kernels' form ca*dy + cb*z + cc, the three vectors stored in coeff_dtype
                ca = gamma * r["rstd"]
                cb = -ca * (dgamma / P) * r["rstd"]
                cc = ca * ((dgamma / P) * r["mean"] * r["rstd"] - dbeta / P)
                ca, cb, cc = (_f64(v.astype(coeff_dtype)) for v in (ca, cb, cc))
                dz = ca * g + cb * r["z"] + cc
            if mutation == "no_constant_term":      # dz = ca*dy + cb*z + cc with cc = 0
                m2 = dgamma / P
                dz = dz - gamma * r["rstd"] * (m2 * r["mean"] * r["rstd"] - dbeta / P)
        else:
            dz = r["scale"] * g
        db = dz.sum(axis=0)
        dz = stored(store, dz)
        h = recs[l - 1]["out"] if l > 0 else _f64(x)
        if l > 0 or store_first:
            h = stored(store, h)
        grads[l] = dict(dw=result(store, dz.T @ h), db=result(store, db), dgamma=dgamma, dbeta=dbeta, dz=dz)
        g = result(store, dz @ stored(store, w))
        if l > 0 and mutation != "dgrad_unmasked":
            g = np.where(masks[l - 1], g, 0.0)
        if l > 0:
            g = stored(store, g)
    return g, grads


def device_masks(z_cat, scale, shift, widths):
    """The masks a kernel takes as fmaf(z, scale, shift) > 0, per layer: the product of two fp32 numbers is exact in
    fp64 and the sum's sign survives its one rounding, so the fp64 expression has the sign of the fused one."""
    off = np.concatenate([[0], np.cumsum(widths)])
    return [_f64(z_cat[:, off[l]:off[l + 1]]) * _f64(scale[off[l]:off[l + 1]]) + _f64(shift[off[l]:off[l + 1]]) > 0
            for l in range(len(widths))]


def band(y, tol, floor=0.0):
    """Half-width of the band around zero in which an error of tol * max(floor, max|y|) can flip a mask."""
    return tol * max(floor, float(np.abs(y).max()))


def band_share(recs, tol, relu_last=0, floor=0.0):
    """Share of the post-BN elements that feed a ReLU with |y| <= tol * max(floor, max|y| of their layer)."""
    L = len(recs)
    inside = total = 0
    for l, r in enumerate(recs):
        if has_relu(l, L, relu_last):
            inside += int((np.abs(r["y"]) <= band(r["y"], tol, floor)).sum())
            total += r["y"].size
    return inside / max(total, 1)


def rel_l2(ref, got):
    ref, got = _f64(ref), _f64(got)
    return float(np.linalg.norm(ref - got) / (np.linalg.norm(ref) + 1e-300))
