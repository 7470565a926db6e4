"""prh_encoder_forward_bf16 / prh_encoder_backward_bf16 (BASELINE config 3) at the C ABI against the bf16-storage
statement of tests/_encoder_ref.py: fp64 arithmetic with a rounding to bf16 exactly where the contract stores or feeds
a 16-bit value (the rounding points are listed in that module's docstring and in include/pointnet_refine_hip.h).  This
is the "kernels compute what they say" check of the pair; tests/test_bf16_gpu.py::test_encoder_bf16_vs_oracle_g3 answers
the other question, whether bf16 is good enough.

Forward, teacher-forced per layer.  The expected z of layer l is computed in fp64 from the DEVICE'S OWN bf16 z of layer
l - 1 and its own scale / shift, so no error is carried from layer to layer.  An element passes iff
    dev in [bf16(ref - band), bf16(ref + band)],   band = GATE_FWD * max(1, max|ref|) of its tensor:
the device stored a correctly rounded value of something within the project's fp32 gate of the reference.  No share of
elements is exempt.  The same holds for `fused` and, with band GATE_FWD, for the stored gate.  mean, rstd, scale, shift
and the running statistics are compared with fp64 statistics of the device's own rounded z, and gfeat's mean half with
the fp64 mean of the device's own `fused`, at today's fp32 gate (fwd_ratio <= 1).  Exact: gfeat's max half is `fused`
at the recorded arg-max bit for bit, the arg-max is the first arg-max of the device's `fused`, the dead channel's is
point 0, num_batches_tracked, and eval mode leaves the running statistics alone.

Backward, as a chain.  dy_f and dy_cat live in the workspace, so the check is the store=bf16 reference as a chain on
the device's saved forward, its exact masks (device_masks on the upcast z) and its arg-max.  dG, read back from
saved.gate, is elementwise work on exactly known inputs: the interval criterion with a band of 8 fp32 ulps of the
product formed with |d| replaced by the sum of the magnitudes of its terms.  Every parameter gradient and d_ctx are
compared by rel-L2 per whole tensor (the training-mode db against sum|dz|) with the gates of
tests/_encoder16_cases.py, which are measured on the CPU from the reference alone: max(1e-5, 4 * what one fp32
evaluation of the chain costs against the fp64 one).  The chain amplifies: an error e in a dgrad's operand flips a
share e / 2^-8 of the next store's roundings, e -> sqrt(e * 2^-8), so the gates run from 1e-4 (fusion) to 2e-2
(conv1, d_ctx): one bf16 ulp is what two correct fp32 evaluations differ by down there.

Every output starts from a sentinel (bf16 NaN bits 0x7FC0 in 16-bit buffers) with guard rows; inputs are cloned and
verified unchanged, saved.gate excepted - the backward is documented to overwrite it with dG.

CPU-derived gates (rel-L2; tests/_encoder16_cases.py):
    fusion.dw 1.5e-4  dgamma 1.0e-4  dbeta 1.1e-4 | conv5 8.0e-4 5.6e-4 8.0e-4 | conv4 2.9e-3 2.6e-3 2.9e-3
    conv3 7.6e-3 7.2e-3 7.6e-3 | conv2 1.3e-2 1.3e-2 1.4e-2 | conv1 1.7e-2 1.8e-2 2.0e-2 | d_ctx 1.6e-2  d_ctx3 1.7e-2
    d_gate_w1 4.8e-5  d_gate_b1 7.6e-5  d_gate_w2 5.2e-5  d_gate_b2 7.2e-5 | every db 1e-5 (of sum|dz| in training)

Largest observed error / gate per quantity over all 11 cases (MI355X; every test prints its own; for the interval
quantities z, gate, fused and dG the figure is (|dev - ref| - half a bf16 ulp) / band, and no element of any case was
outside its interval):
    z 0.003  mean 0.003  rstd 0.006  scale 0.005  shift 0.008  running_mean 0.001  running_var 0.003  gate 0.001
    fused 0.000  gfeat_mean 0.003  |  dG 0.171
    layer    dw      dgamma  dbeta   db
    fusion   0.801   0.241   0.245   0.001      (0.801: tails_eval, P = 35; training cases stay at or below 0.288)
    conv5    0.311   0.369   0.269   0.241      (db: the eval cases, against dbeta's gate; training 0.000)
    conv4    0.321   0.314   0.265   0.095
    conv3    0.270   0.251   0.263   0.051
    conv2    0.234   0.241   0.223   0.037
    conv1    0.279   0.238   0.226   0.033
    d_ctx 0.254  d_ctx3 0.256  d_gate_w1 0.296  d_gate_b1 0.719  d_gate_w2 0.273  d_gate_b2 0.786 (both od512)
The chained quantities sit near a quarter of their gates - a device evaluation differs from the fp64 chain by about
what the CPU's fp32 evaluation does, as the factor 4 intends - and no ratio is above 1: no finding, no gate widened,
no rounding point of the issue's reading had to be corrected but one: db is formed from the two BatchNorm sums
(bn_bwd_finalize_kernel: a*Sdy + b*P*mean + c*P), i.e. it is the sum of the UNROUNDED dz, not of the stored one.
Mask flips against the reference's own free-running store=bf16 forward (bf16 noise on the way, not a check) and
arg-max differences, per case: small 36 / 8, small_eval 1 / 0, tails 0 / 0, tails_eval 0 / 0, c12 1 / 0, od512 51 / 3,
mid 856 / 7, mid_pool (all three) 665 / 16 (fused_only: no arg-max), od2048 229 / 6.  The backward always runs on the
device's own masks and arg-max, which the test rebuilds exactly.

A defect that belongs with this work and is fixed with it: prh_encoder_backward_bf16 refused d_ctx at in_channel % 4
!= 0 (C = 6 is BASELINE config 4) in front of its LAST conv launch, after saved.gate had been overwritten with dG and
most gradients written; a fusion conv too deep for its prologue image (out_dim > 3008) was refused after the five
convs had run; and the backward tested no width at all.  Every shape refusal now comes before the device is touched;
the refusal tests below were only ever run against the fixed library.
"""
import ctypes as C

import numpy as np
import pytest
import torch

import _encoder16_cases as K16
import _encoder_cases as K
import _encoder_ref as E
import _stack_ref as S

pytestmark = pytest.mark.gpu

GUARD = 4                         # sentinel rows in front of and behind every output
PRH_ERR_ARG = -1
INT_SENTINEL = -7
BF16_NAN = 0x7FC0
COEF = ("scale", "shift", "mean", "rstd")
LAYERS = [f"conv{k}" for k in range(1, 6)] + ["fusion"]
GATE_GRADS = ("d_gate_w1", "d_gate_b1", "d_gate_w2", "d_gate_b2")


# ------------------------------------------------------------------------------------------ plumbing
def _p(t):
    return C.c_void_p(0 if t is None or t.numel() == 0 else t.data_ptr())


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _guarded(rows, width, dtype=torch.float32):
    """A (rows, width) view of sentinels (NaN; bf16 NaN bits in int16; INT_SENTINEL in int32) with GUARD sentinel
    rows on either side; returns (view, whole)."""
    fill = float("nan") if dtype.is_floating_point else (BF16_NAN if dtype == torch.int16 else INT_SENTINEL)
    whole = torch.full((rows + 2 * GUARD, width), fill, dtype=dtype, device="cuda")
    return whole[GUARD:GUARD + rows], whole


def _untouched(t):
    if t.dtype.is_floating_point:
        return bool(torch.isnan(t).all())
    return bool((t == (BF16_NAN if t.dtype == torch.int16 else INT_SENTINEL)).all())


def _guards_intact(whole):
    return _untouched(whole[:GUARD]) and _untouched(whole[-GUARD:])


def _vec(width):
    v, whole = _guarded(1, width)
    return v[0], whole


def _same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(a.contiguous().view(torch.uint8), b.contiguous().view(torch.uint8))


def _np(t):
    return t.detach().cpu().numpy()


def _up(t):
    """A device buffer of bf16 bits as fp64."""
    return K16.from_bits16(_np(t).view(np.uint16))


def _worst(a, b):
    return float("nan") if a != a or b != b else max(a, b)


def _inside(ref, dev, band):
    """dev in [bf16(ref - band), bf16(ref + band)] per element, and for the printed table the largest
    (|dev - ref| - half a bf16 ulp of dev) / band: <= 1 where the criterion holds, up to ties."""
    ok = (dev >= S.bf16(ref - band)) & (dev <= S.bf16(ref + band))
    half_ulp = np.ldexp(1.0, np.frexp(dev)[1] - 9)
    with np.errstate(divide="ignore", invalid="ignore"):
        t = np.where(band > 0, np.maximum(np.abs(dev - ref) - half_ulp, 0.0) / band, np.where(dev == ref, 0.0, np.inf))
    return int((~ok).sum()), float(np.max(t)) if np.isfinite(dev).all() else float("nan")


@pytest.fixture()
def lib16():
    from pointnet_refine_amd import _lib
    lib = _lib.lib()
    old = lib.prh_get_gemm_mode()
    assert lib.prh_set_gemm_mode(4) == 0
    yield lib
    lib.prh_set_gemm_mode(old)


class Encoder16:
    """Device copies of an input set and the two bf16 entry points around them.  shapes_only: zero weights of the
    given widths, for calls that must be refused before anything is read."""

    def __init__(self, lib, key, shapes_only=False):
        self.lib, self.key = lib, key
        self.C, self.B, self.N, self.od, self.training = key
        self.P, self.cat = self.B * self.N, sum(E.CONV_WIDTHS) + self.od
        w = (self.C,) + E.CONV_WIDTHS + (self.od,)
        p2 = [None] * 28                                  # ops.ENC_PARAM_ORDER
        if shapes_only:
            z = lambda *s: torch.zeros(*s, device="cuda")
            for l in range(5):
                p2[2 * l], p2[2 * l + 1], p2[10 + 2 * l], p2[11 + 2 * l] = z(w[l + 1], w[l]), z(w[l + 1]), z(w[l + 1]), z(w[l + 1])
            p2[20:24] = [z(self.od, self.cat), z(self.od), z(self.od), z(self.od)]
            p2[24:28] = [z(64, 1), z(64), z(self.od, 64), z(self.od)]
            self.bufs0 = [t for l in range(6) for t in (z(w[min(l, 4) + 1]), z(w[min(l, 4) + 1]) + 1,
                                                        torch.tensor(K.NBT0 + l, dtype=torch.int64, device="cuda"))]
            self.ctx = z(self.B, self.N, self.C)
            self.d_fused = torch.zeros(self.P, self.od, dtype=torch.int16, device="cuda")
            self.d_gfeat = z(self.B, 2 * self.od)
        else:
            prm, running, ctx, _, d_gfeat = K.inputs(key)
            dev = lambda a: torch.from_numpy(np.array(a)).cuda()
            layers = prm["conv"] + [prm["fusion"]]
            for l in range(5):
                p2[2 * l], p2[2 * l + 1] = dev(layers[l]["w"]), dev(layers[l]["b"])
                p2[10 + 2 * l], p2[11 + 2 * l] = dev(layers[l]["gamma"]), dev(layers[l]["beta"])
            p2[20:24] = [dev(prm["fusion"][k]) for k in ("w", "b", "gamma", "beta")]
            p2[24:28] = [dev(prm["w1"]).reshape(64, 1), dev(prm["b1"]), dev(prm["w2"]), dev(prm["b2"])]
            self.bufs0 = [t for l, (rm, rv) in enumerate(running)
                          for t in (dev(rm), dev(rv), torch.tensor(K.NBT0 + l, dtype=torch.int64, device="cuda"))]
            self.ctx = dev(ctx).reshape(self.B, self.N, self.C)
            self.d_fused = dev(K16.bits16(K16.d_fused16(key)).view(np.int16))
            self.d_gfeat = dev(d_gfeat)
        self.p2 = p2

    def workspace(self, backward):
        n = int(self.lib.prh_encoder_bf16_workspace_bytes(self.B, self.N, self.C, self.od, backward))
        return torch.empty(n, dtype=torch.uint8, device="cuda")

    def forward(self, pooled=True):
        from pointnet_refine_amd import _lib as L, ops
        P, od, cat, B = self.P, self.od, self.cat, self.B
        bufs = [t.clone() for t in self.bufs0]
        out = dict(training=self.training, bufs=bufs, gfeat=None, argmax=None)
        wholes = []
        for k, w in (("z_cat", cat), ("z_fus", od), ("fused", od), ("gate", od)):
            out[k], whole = _guarded(P, w, torch.int16)
            wholes.append(whole)
        for k in COEF:
            out[k], whole = _vec(cat + od)
            wholes.append(whole)
        if pooled:
            out["gfeat"], whole = _guarded(B, 2 * od)
            out["argmax"], whole_i = _guarded(B, od, torch.int32)
            wholes += [whole, whole_i]
        out["wholes"] = wholes
        prm = ops._enc_params_struct(self.p2, bufs, self.C)
        sv = L.EncoderSavedBf16(_p(out["z_cat"]), _p(out["z_fus"]), _p(out["gate"]), _p(out["scale"]), _p(out["shift"]),
                                _p(out["mean"]), _p(out["rstd"]), _p(out["argmax"]))
        ws = self.workspace(0)
        rc = self.lib.prh_encoder_forward_bf16(C.byref(prm), _p(self.ctx), B, self.N, self.training, K.MOMENTUM, K.EPS,
                                               _p(out["fused"]), _p(out["gfeat"]), C.byref(sv), _p(ws), ws.numel(), 0, _stream())
        torch.cuda.synchronize()
        return rc, out

    def backward(self, fw, d_fused=True, d_gfeat=True, null=(), want_dctx=True):
        """null: names of gradient pointers passed as NULL ("conv2.dw", "fusion.dgamma", "d_gate_w1", ...).  fw: the
        forward's outputs, or None (refusal tests: sentinels stand in for a saved forward)."""
        from pointnet_refine_amd import _lib as L, ops
        P, od, cat = self.P, self.od, self.cat
        wholes = []
        gate, gate_whole = _guarded(P, od, torch.int16)
        if fw is None:
            fw = {k: _guarded(P, w, torch.int16)[0] for k, w in (("z_cat", cat), ("z_fus", od))}
            fw.update({k: _vec(cat + od)[0] for k in COEF}, argmax=_guarded(self.B, od, torch.int32)[0], training=self.training)
        else:
            gate.copy_(fw["gate"])
        sv = L.EncoderSavedBf16(_p(fw["z_cat"]), _p(fw["z_fus"]), _p(gate), _p(fw["scale"]), _p(fw["shift"]),
                                _p(fw["mean"]), _p(fw["rstd"]), _p(fw["argmax"]))
        got = dict(conv=[], dG=gate, gate_whole=gate_whole, gate_before=gate.clone())
        gr = L.EncoderGrads()
        for l, name in enumerate(LAYERS):
            w = self.p2[2 * l] if l < 5 else self.p2[20]
            g = dict(zip(("db", "dgamma", "dbeta"), (_vec(w.shape[0]) for _ in range(3))))
            g["dw"] = _guarded(*w.shape)
            wholes += [v[1] for v in g.values()]
            g = {k: v[0] for k, v in g.items()}
            st = L.BnLayerGrad(*[_p(None if f"{name}.{k}" in null else g[k]) for k in ("dw", "db", "dgamma", "dbeta")])
            if l < 5:
                gr.conv[l] = st
                got["conv"].append(g)
            else:
                gr.fusion = st
                got["fusion"] = g
        for k, i in zip(GATE_GRADS, (24, 25, 26, 27)):
            t, whole = _guarded(self.p2[i].shape[0], self.p2[i].shape[1] if self.p2[i].dim() == 2 else 1)
            wholes.append(whole)
            got[k] = t.reshape(self.p2[i].shape)
            setattr(gr, k, _p(None if k in null else t))
        got["d_ctx"], whole = _guarded(P, self.C)
        wholes.append(whole)
        got["wholes"] = wholes
        prm = ops._enc_params_struct(self.p2, None, self.C)
        ws = self.workspace(1)
        rc = self.lib.prh_encoder_backward_bf16(C.byref(prm), _p(self.ctx), self.B, self.N, fw["training"],
                                                _p(self.d_fused if d_fused else None), _p(self.d_gfeat if d_gfeat else None),
                                                C.byref(sv), C.byref(gr), _p(got["d_ctx"] if want_dctx else None), _p(ws),
                                                ws.numel(), 0, _stream())
        torch.cuda.synchronize()
        return rc, got

    def outputs_untouched(self, fw=None, bw=None):
        """No launch wrote anything: every output still holds its sentinels, the statistics their initial values and
        saved.gate what it held."""
        ok = True
        if fw is not None:
            ok = ok and all(_untouched(w) for w in fw["wholes"])
            ok = ok and all(torch.equal(a, b) for a, b in zip(fw["bufs"], self.bufs0))
        if bw is not None:
            ok = ok and all(_untouched(w) for w in bw["wholes"]) and _same(bw["dG"], bw["gate_before"])
            ok = ok and _guards_intact(bw["gate_whole"])
        return ok


def _grads_np(bw):
    f = lambda g: {k: _np(v) for k, v in g.items()}
    return dict(d_ctx=_np(bw["d_ctx"]), conv=[f(g) for g in bw["conv"]], fusion=f(bw["fusion"]),
                **{k: _np(bw[k]).reshape(-1) if k != "d_gate_w2" else _np(bw[k]) for k in GATE_GRADS})


def _grad_tensors(bw, skip=()):
    t = {"d_ctx": bw["d_ctx"], **{k: bw[k] for k in GATE_GRADS}}
    for name, g in zip(LAYERS, bw["conv"] + [bw["fusion"]]):
        t.update({f"{name}.{k}": v for k, v in g.items()})
    return {k: v for k, v in t.items() if k not in skip}


def _check_forward(en, fw, pooled):
    """Error / gate of every forward quantity (<= 1 passes; the interval quantities z, fused, gate also count their
    elements outside), the device's saved forward in fp64, its masks, and the list of hard failures."""
    od, cat, B, N, P, bad = en.od, en.cat, en.B, en.N, en.P, []
    prm, running, ctx, _, _ = K.inputs(en.key)
    if not all(_guards_intact(w) for w in fw["wholes"]):
        bad.append("forward wrote into a guard row")
    z_cat, z_fus, fused, gate = (_up(fw[k]) for k in ("z_cat", "z_fus", "fused", "gate"))
    co = {k: _np(fw[k]).astype(np.float64) for k in COEF}
    dm = E.device_masks(ctx, prm, z_cat, z_fus, co["scale"], co["shift"], od, _np(fw["argmax"]) if pooled else None)
    q = dict(z=0.0, mean=0.0, rstd=0.0, scale=0.0, shift=0.0, running_mean=0.0, running_var=0.0)
    off = np.concatenate([[0], np.cumsum(list(E.CONV_WIDTHS) + [od, od])])
    outside = 0
    acts = []                     # A of the next layer, from the device's own z, scale and shift, as the prologue stores it
    for l, ly in enumerate(prm["conv"] + [prm["fusion"]]):
        s = slice(off[l], off[l + 1])
        z = z_cat[:, s] if l < 5 else z_fus
        w, b = np.asarray(ly["w"], np.float64), np.asarray(ly["b"], np.float64)
        if l == 0:
            x = np.asarray(ctx, np.float64)
            ref = S.bf16(x) @ S.bf16(w).T + b if E.store_first(en.C) else x @ w.T + b
        else:
            ref = (acts[l - 1] if l < 5 else np.concatenate(acts, axis=1)) @ S.bf16(w).T + b
        n_out, t = _inside(ref, z, K.GATE_FWD * max(1.0, float(np.abs(ref).max())))
        outside += n_out
        q["z"] = _worst(q["z"], t)
        bn = S.batchnorm(z, ly, running[l], fw["training"], K.MOMENTUM, K.EPS)
        for k in COEF:
            q[k] = _worst(q[k], K.fwd_ratio(bn[k], co[k][s]))
        rm, rv, nbt = fw["bufs"][3 * l:3 * l + 3]
        if fw["training"]:
            q["running_mean"] = _worst(q["running_mean"], K.fwd_ratio(bn["running_mean"], _np(rm)))
            q["running_var"] = _worst(q["running_var"], K.fwd_ratio(bn["running_var"], _np(rv)))
        elif not (_same(rm, en.bufs0[3 * l]) and _same(rv, en.bufs0[3 * l + 1])):
            bad.append(f"eval mode touched the running statistics of layer {l}")
        want = K.NBT0 + l + (1 if fw["training"] else 0)
        if int(nbt) != want:
            bad.append(f"num_batches_tracked of layer {l}: {int(nbt)}, expected {want}")
        if l < 5:
            acts.append(S.BF16_VIA_F32(np.maximum(z * co["scale"][s] + co["shift"][s], 0.0)))
    if outside:
        bad.append(f"{outside} elements of z outside their interval")
    g = E.gate(ctx, prm, store=S.BF16_VIA_F32)                       # u and W2 as stored; the hidden layer is fp32 inputs alone
    m = 0.5 + 0.5 * g["sig"]
    n_out, q["gate"] = _inside(m, gate, K.GATE_FWD)
    if n_out:
        bad.append(f"{n_out} elements of the stored gate outside their interval")
    s = slice(cat, cat + od)
    ref = np.maximum(z_fus * co["scale"][s] + co["shift"][s], 0.0) * m
    n_out, q["fused"] = _inside(ref, fused, K.GATE_FWD * max(1.0, float(np.abs(ref).max())))
    if n_out:
        bad.append(f"{n_out} elements of fused outside their interval")
    if fused[:, K.DEAD].any():
        bad.append("the dead channel of fused is not zero")
    if pooled:
        gfeat, arg = _np(fw["gfeat"]), _np(fw["argmax"]).astype(np.int64)
        Fb = fused.reshape(B, N, od)
        q["gfeat_mean"] = K.fwd_ratio(Fb.mean(axis=1), gfeat[:, od:])
        if not np.array_equal(arg, np.argmax(Fb, axis=1)):
            bad.append("argmax is not the first arg-max of the device's own fused")
        elif not np.array_equal(gfeat[:, :od].view(np.int32),
                                np.take_along_axis(Fb, arg[:, None, :], axis=1)[:, 0].astype(np.float32).view(np.int32)):
            bad.append("gfeat's max half is not fused at argmax, bit for bit")
        if arg[:, K.DEAD].any():
            bad.append("the dead channel's arg-max is not point 0")
    sf = dict(z_cat=z_cat, z_fus=z_fus, gate=gate, fused=fused, **co)
    return q, sf, dm, bad


def _reference_chain(en, fw, sf, dm, d_fused, d_gfeat):
    prm, running, ctx, _, dg = K.inputs(en.key)
    conv, fus = E.records_from_saved(sf["z_cat"], sf["z_fus"], sf["scale"], sf["shift"], sf["mean"], sf["rstd"], en.od, dm)
    dF = K16.d_fused16(en.key) if d_fused else None
    dg = dg if d_gfeat else None
    ref = E.backward(dF, dg, ctx, en.B, en.N, prm, conv, fus, fw["training"], dm, store=S.BF16, m_saved=sf["gate"])
    # the elementwise dG: the product before its store, and its band of DG_ULPS fp32 ulps of the product of magnitudes
    d, mag = E.pooled_terms(dF, dg, en.B, en.N, en.od, dm["argmax"])
    sig = 2.0 * sf["gate"] - 1.0
    fac = np.where(dm["fus"], fus["y"], 0.0) * 0.5 * sig * (1.0 - sig)
    band = K16.DG_ULPS * np.spacing((mag * np.abs(fac)).astype(np.float32)).astype(np.float64)
    return ref, d * fac, band


def _verdict(tag, q, bad, limits):
    print(tag, " ".join(f"{k}={v / limits.get(k, 1.0):.3f}" for k, v in q.items()), "|", "; ".join(bad) if bad else "ok")
    over = {k: round(v / limits.get(k, 1.0), 3) for k, v in q.items() if not v <= limits.get(k, 1.0)}
    assert not bad and not over, (tag, bad, over)


# ------------------------------------------------------------------------------------------ the cases
@pytest.mark.parametrize("case", K16.CASES, ids=[c.id for c in K16.CASES])
def test_encoder_bf16_forward_and_backward_against_the_stored_reference(lib16, case):
    lib = lib16
    en = Encoder16(lib, case.inputs)
    rc, fw = en.forward(pooled=case.pooled)
    assert rc == 0, lib.prh_last_error()
    qf, sf, dm, bad = _check_forward(en, fw, case.pooled)
    # for the table only: how far the device's decisions are from the reference's own free-running bf16 forward
    own = K16.saved_forward(case.inputs)
    flips = sum(int((a != b).sum()) for a, b in zip(dm["conv"] + [dm["fus"]], [r["mask"] for r in own["conv"]] + [own["fus"]["mask"]]))
    argdiff = int((dm["argmax"] != own["argmax"]).sum()) if case.pooled else 0
    ref, dG_ref, dG_band = _reference_chain(en, fw, sf, dm, case.d_fused, case.d_gfeat)
    keep = {k: fw[k].clone() for k in ("z_cat", "z_fus") + COEF + (("argmax",) if case.pooled else ())}
    rc, bw = en.backward(fw, case.d_fused, case.d_gfeat, want_dctx=bool(case.d_ctx))
    assert rc == 0, lib.prh_last_error()
    got = _grads_np(bw)
    if not case.d_ctx:
        if not torch.isnan(bw["d_ctx"]).all():
            bad.append("d_ctx = NULL and its buffer was written")
        got["d_ctx"] = ref["d_ctx"]
    qb = K16.quantities(ref, got, fw["training"])
    if not case.d_ctx:
        del qb["d_ctx"], qb["d_ctx3"]
    n_out, qb["dG"] = _inside(dG_ref, _up(bw["dG"]), dG_band)
    if n_out:
        bad.append(f"{n_out} elements of dG outside their interval")
    if not all(_guards_intact(w) for w in bw["wholes"] + [bw["gate_whole"]]):
        bad.append("backward wrote into a guard row")
    prm, running, ctx, _, d_gfeat = K.inputs(case.inputs)
    if not (all(_same(keep[k], fw[k]) for k in keep) and np.array_equal(_np(en.ctx).reshape(-1, case.C), ctx)
            and np.array_equal(_np(en.d_gfeat), d_gfeat)
            and np.array_equal(_np(en.d_fused).view(np.uint16), K16.bits16(K16.d_fused16(case.inputs)))):
        bad.append("the backward changed one of its inputs")
    if not fw["training"] and not all(np.abs(_np(g["db"])).max() > 0 for g in bw["conv"] + [bw["fusion"]]):
        bad.append("an eval-mode db is zero")
    _verdict(f"ENC16 {case.id} flips={flips} argdiff={argdiff}", {**qf, **qb}, bad, K16.limits(fw["training"]))


# ------------------------------------------------------------------------------------------ contract edges
SMALL = K16.BY_ID["small_train"]
TAILS = K16.BY_ID["tails_train"]


def test_null_gradient_pointers_and_null_d_ctx_leave_the_rest_bit_equal(lib16):
    lib = lib16
    en = Encoder16(lib, SMALL.inputs)
    rc, fw = en.forward()
    assert rc == 0, lib.prh_last_error()
    rc, full = en.backward(fw)
    assert rc == 0, lib.prh_last_error()
    null = ("conv1.db", "conv1.dw", "conv2.dw", "conv3.dbeta", "fusion.dw", "fusion.dgamma", "d_gate_w1", "d_gate_b1")
    rc, part = en.backward(fw, null=null)
    assert rc == 0, lib.prh_last_error()
    tf, tp = _grad_tensors(full), _grad_tensors(part)
    assert all(torch.isnan(tp[k]).all() for k in null)
    assert all(_same(tf[k], tp[k]) for k in tf if k not in null), [k for k in tf if k not in null and not _same(tf[k], tp[k])]
    rc, no_dx = en.backward(fw, want_dctx=False)
    assert rc == 0, lib.prh_last_error()
    tn = _grad_tensors(no_dx, skip=("d_ctx",))
    assert torch.isnan(no_dx["d_ctx"]).all() and all(_same(tf[k], tn[k]) for k in tn)
    assert _same(full["dG"], part["dG"]) and _same(full["dG"], no_dx["dG"])
    assert all(_guards_intact(w) for w in part["wholes"] + no_dx["wholes"])


def test_d_ctx_at_six_channels_is_refused_before_anything_is_written(lib16):
    """d_ctx needs in_channel % 4 == 0 (fp32 vector stores of the conv1 dgrad), and C = 6 is BASELINE config 4's channel
    count.  The refusal used to sit in front of that last launch: every earlier one had run, saved.gate was overwritten
    with dG and most gradients were written.  It now comes before the device is touched."""
    lib = lib16
    en = Encoder16(lib, TAILS.inputs)
    rc, fw = en.forward()
    assert rc == 0, lib.prh_last_error()
    rc, bw = en.backward(fw, want_dctx=True)
    assert rc == PRH_ERR_ARG and b"in_channel % 4" in lib.prh_last_error(), lib.prh_last_error()
    assert en.outputs_untouched(bw=bw)
    rc, bw = en.backward(fw, want_dctx=False)
    assert rc == 0, lib.prh_last_error()
    assert not any(torch.isnan(v).any() for v in _grad_tensors(bw, skip=("d_ctx",)).values()) and torch.isnan(bw["d_ctx"]).all()


def test_shapes_the_launches_would_refuse_are_refused_before_anything_is_written(lib16):
    """The other shape refusals reachable inside the two entry points: a fusion conv too deep for the LDS image of its
    BN+ReLU prologue (K = cat <= 3968, out_dim <= 3008 - the five convs had run by then), and a width that is no
    multiple of 8, which the backward did not test at all (its step 1 ran, then the first wgrad refused)."""
    lib = lib16
    deep = Encoder16(lib, (4, 1, 16, 3016, 1), shapes_only=True)
    assert K16.nt_b16_lds(deep.cat, True) > 160 * 1024
    rc, fw = deep.forward()
    assert rc == PRH_ERR_ARG and b"prologue coefficient image" in lib.prh_last_error(), lib.prh_last_error()
    assert deep.outputs_untouched(fw=fw)
    rc, bw = deep.backward(None)
    assert rc == PRH_ERR_ARG and b"prologue coefficient image" in lib.prh_last_error(), lib.prh_last_error()
    assert deep.outputs_untouched(bw=bw)
    odd = Encoder16(lib, (4, 1, 16, 132, 1), shapes_only=True)
    rc, fw = odd.forward()
    assert rc == PRH_ERR_ARG and b"of 8" in lib.prh_last_error() and odd.outputs_untouched(fw=fw)
    rc, bw = odd.backward(None)
    assert rc == PRH_ERR_ARG and b"of 8" in lib.prh_last_error() and odd.outputs_untouched(bw=bw)
