"""fp64 numpy reference of a shared-MLP stack: L layers of Linear + BatchNorm1d (+ ReLU), forward and backward.

A layer is a dict(w [cout, cin], b, gamma, beta); `running` is a list of (running_mean, running_var).  Every array is
taken to fp64 on entry.  Layer l is followed by a ReLU when l < L - 1 or relu_last is set.  The ReLU is written as
where(mask, y, 0) so that masks taken elsewhere - from the device's own z, scale and shift (device_masks) - can stand
in for the layer's own y > 0: with the masks fixed the stack is Linear + BatchNorm only, and two evaluations differ by
arithmetic error alone.  No torch, no GPU.
"""
import numpy as np

MUTATIONS = ("no_constant_term", "biased_running_var", "relu_last_ignored", "dgrad_unmasked")


def _f64(a):
    return np.asarray(a, dtype=np.float64)


def has_relu(l, L, relu_last):
    return l < L - 1 or bool(relu_last)


def forward(x, layers, training, momentum, eps, relu_last, running, masks=None, mutation=None):
    """Per layer: z, mean, rstd (biased variance), scale, shift, y (post-BN), running_mean / running_var after the call
    (unbiased variance, as nn.BatchNorm1d; unchanged in eval), mask (the layer's own y > 0) and out.
    mutation: one of MUTATIONS, a deliberate mistake (tests/test_stack_ref_cpu.py shows the inputs detect each)."""
    L = len(layers)
    h = _f64(x)
    P = h.shape[0]
    recs = []
    for l, ly in enumerate(layers):
        w, b, gamma, beta = (_f64(ly[k]) for k in ("w", "b", "gamma", "beta"))
        rm, rv = _f64(running[l][0]), _f64(running[l][1])
        z = h @ w.T + b
        if training:
            mean = z.mean(axis=0)
            m2 = ((z - mean) ** 2).sum(axis=0)
            rstd = 1.0 / np.sqrt(m2 / P + eps)
            new_rm = (1.0 - momentum) * rm + momentum * mean
            new_rv = (1.0 - momentum) * rv + momentum * (m2 / (P if mutation == "biased_running_var" else P - 1))
        else:
            mean, rstd, new_rm, new_rv = rm, 1.0 / np.sqrt(rv + eps), rm, rv
        scale = gamma * rstd
        shift = beta - mean * scale
        y = z * scale + shift
        own = y > 0
        if has_relu(l, L, relu_last):
            out = np.where(own if masks is None else masks[l], y, 0.0)
        else:
            out = y
        recs.append(dict(z=z, mean=mean, rstd=rstd, scale=scale, shift=shift, y=y, running_mean=new_rm,
                         running_var=new_rv, mask=own, out=out))
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


def backward(dy, x, layers, recs, training, relu_last, masks, mutation=None, coeff_dtype=None):
    """dx and, per layer, dw, db, dgamma, dbeta (and dz, for the tests' scales) from the records of a forward.
    Training: the full BatchNorm backward.  Eval: dz = scale * dy.
    coeff_dtype: round the three BatchNorm-backward coefficient vectors to this type and nothing else - what storing
    them in fp32 alone costs (at P = 2 the terms of dz cancel to eps / (var + eps) of themselves)."""
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
        dbeta = g.sum(axis=0)
        dgamma = (g * xhat).sum(axis=0)
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
        h = recs[l - 1]["out"] if l > 0 else _f64(x)
        grads[l] = dict(dw=dz.T @ h, db=dz.sum(axis=0), dgamma=dgamma, dbeta=dbeta, dz=dz)
        g = dz @ w
        if l > 0 and mutation != "dgrad_unmasked":
            g = np.where(masks[l - 1], g, 0.0)
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
