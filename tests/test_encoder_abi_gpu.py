"""prh_encoder_forward / prh_encoder_backward at the C ABI against the fp64 reference of tests/_encoder_ref.py.

The backward is compared on the DEVICE'S OWN MASKS: every kernel decides a ReLU as fmaf(z, scale, shift) > 0 (the gate
hidden layer as fmaf(inten, w1, b1) > 0) and the forward returns z_cat, z_fus, bn_scale, bn_shift and the arg-max, so
the test recomputes each mask exactly (_encoder_ref.device_masks) and runs the reference backward on the device's saved
forward with the device's masks and arg-max.  The gate m is always the reference's own, in fp64, from ctx and the
weights.  What is left between the two is arithmetic error, and the gates are the project's own for these GEMM cores:
forward max-abs 2e-5 * max(1, max|ref|), gradients rel-L2 1e-5 per tensor, shared by modes 0, 1 and 3.  The
training-mode db is analytically zero and is measured against sum|dz| of its columns.  The forward is compared with
the reference on its own masks; device masks may differ from those only where |y_ref| <= 2e-5 * max(1, max|y_ref|) of
the layer, and the recorded arg-max is the first arg-max of the device's own `fused`, exactly.

Cases (tests/_encoder_cases.py) are the smallest sizes that select each path of the two entry points;
test_the_cases_select_the_kernel_families_they_are_named_for restates the library's rules.  Every output starts from
NaN with guard rows in front and behind; running statistics and counters are cloned per call; momentum = 0.25 and
eps = 3e-5 throughout.

Largest observed error / gate per quantity and mode over all 19 cases (MI355X; every test prints its own).  conv.*
is the largest over conv1..5, d_ctx3 is column 3 of d_ctx on its own:
    mode 0:  z 0.062  y 0.077  mean 0.009  rstd 0.027  scale 0.023  shift 0.022  running_mean 0.004  running_var 0.006
             fused 0.088  gate 0.006  gfeat 0.088  |  d_ctx 0.102  d_ctx3 0.108  conv.dw 0.106  conv.dgamma 0.116
             conv.dbeta 0.105  conv.db 0.033  fusion.dw 0.028  fusion.dgamma 0.016  fusion.dbeta 0.019  fusion.db 0.009
             d_gate_w1 0.045  d_gate_b1 0.054  d_gate_w2 0.026  d_gate_b2 0.017
    mode 1:  z 0.062  y 0.079  mean 0.009  rstd 0.027  scale 0.023  shift 0.022  running_mean 0.004  running_var 0.006
             fused 0.090  gate 0.008  gfeat 0.088  |  d_ctx 0.102  d_ctx3 0.108  conv.dw 0.145  conv.dgamma 0.490
             conv.dbeta 0.787  conv.db 0.001  fusion.dw 0.060  fusion.dgamma 0.019  fusion.dbeta 0.023  fusion.db 0.001
             d_gate_w1 0.054  d_gate_b1 0.056  d_gate_w2 0.027  d_gate_b2 0.019
    mode 3:  z 0.070  y 0.087  mean 0.009  rstd 0.027  scale 0.023  shift 0.022  running_mean 0.004  running_var 0.006
             fused 0.088  gate 0.008  gfeat 0.088  |  d_ctx 0.102  d_ctx3 0.108  conv.dw 0.204  conv.dgamma 0.351
             conv.dbeta 0.400  conv.db 0.260  fusion.dw 0.064  fusion.dgamma 0.025  fusion.dbeta 0.024  fusion.db 0.023
             d_gate_w1 0.046  d_gate_b1 0.058  d_gate_w2 0.029  d_gate_b2 0.027
The largest ratio anywhere is 0.787 (dbeta of conv4, big_both on the first-generation split-bf16 cores); mode 3 stays
at or below 0.40; the eval-mode db (not analytically zero) is the 0.260.  Every mode keeps its claim of fp32-level accuracy;
no gate was widened.  Mask flips against the reference's own masks: 16 elements in all 19 cases together (mid_pool 3,
big_recompute 3, big_both 2 and 3, big_c6 4, big_pool 1), every one inside the band; the gate hidden mask, a function
of the fp32 inputs alone, never differs.  Arg-max differences against the reference's own: 1 (segment, channel) pair
(small_eval), within twice the band of the reference maximum.  Band shares of the inputs (asserted <= 1e-3 by
tests/test_encoder_ref_cpu.py): conv and fusion layers 5.2e-5 to 4.0e-4, gate hidden layer at most 9.5e-6.

No quantity has a gate of its own (_encoder_cases.OWN_GATES is empty).  The one candidate was the fp32 stored gate:
the contract keeps m = 0.5 + 0.5*sig in fp32 and forms sig = 2m - 1, and 1 - sig cancels near saturation
(pre-activations reach 12 here).  Rounding m alone in the fp64 reference costs at most rel-L2 1.4e-7 on d_gate_w2,
1.3e-7 on d_gate_w1, 5.4e-8 on d_gate_b1, 4.3e-8 on d_gate_b2 and 2.6e-8 on d_ctx[:, 3]
(test_what_the_fp32_stored_gate_costs): 0.014 gates, and the device's gate gradients sit at 0.06 gates and below.

A defect that belongs with this work and is fixed with it: the four encoder entry points (fp32 and bf16 storage)
tested the workspace carve alone, so a NULL workspace with a non-zero size passed - every carved pointer NULL - and so
did a workspace up to 256 bytes short.  They now follow the rule of the bf16 Linear and the stack entry points
(present, and no smaller than *_workspace_bytes reports) and refuse before the device is touched; the refusal tests
below were only ever run against the fixed library.
"""
import ctypes as C

import numpy as np
import pytest
import torch

import _encoder_cases as K
import _encoder_ref as E
import _stack_ref as S

pytestmark = pytest.mark.gpu

GUARD = 4                         # sentinel rows in front of and behind every output (4 rows keep 16-byte alignment)
PRH_ERR_ARG, PRH_ERR_WORKSPACE = -1, -2
INT_SENTINEL = -7
COEF = ("scale", "shift", "mean", "rstd")
LAYERS = [f"conv{k}" for k in range(1, 6)] + ["fusion"]
GATE_GRADS = ("d_gate_w1", "d_gate_b1", "d_gate_w2", "d_gate_b2")


def test_the_cases_select_the_kernel_families_they_are_named_for():
    """csrc/prh_lib.hip's launch rules restated (tests/_encoder_cases.py, tests/_stack_cases.py), so that a moved
    threshold does not silently turn these cases into repeats of one another.  fwd: conv1..5, fusion, gate; h2:
    second-generation split-fp16 NT core, h2tr: its transposed-read TN core, "+apply": held back to carry the apply
    pass of the layer below, s3: split-bf16 (first generation)."""
    f = {c.id: K.families(c) for c in K.CASES}
    fp32_7, fp32_5 = ("fp32",) * 7, ("fp32",) * 5
    for cid in ("small_m0_train", "small_m1_train", "small_m3_train", "small_eval_m3_eval", "tails_m0_train",
                "tails_m3_train", "tails_m0_eval", "tails_m3_eval"):
        assert f[cid]["fwd"] == fp32_7 and f[cid]["fusion"] == ("fp32", "fp32") and f[cid]["pool"] == "kernel", cid
        assert f[cid]["conv_dgrad"] == fp32_5 and f[cid]["conv_wgrad"] == fp32_5 and not f[cid]["recompute_ok"], cid
        assert f[cid]["mat"] == cid.split("_")[-2].endswith("m3"), cid      # dz materialised in mode 3, od % 4 == 0
    # P = 2049: nine row tiles, so only the 1024-wide launches reach the 32-tile floor of the split cores
    mid_fwd = ("fp32",) * 4 + ("h2",) * 3
    for cid in ("mid_recompute_m3_train", "mid_stored_m3_train", "mid_eval_m3_eval", "mid_pool_m3_train"):
        assert f[cid]["fwd"] == mid_fwd and f[cid]["fusion"] == ("fp32", "h2") and f[cid]["recompute_ok"], cid
        assert f[cid]["conv_dgrad"] == fp32_5 and f[cid]["conv_wgrad"] == fp32_5 and f[cid]["mat"], cid   # 512 wide: 18 tiles
    assert f["mid_recompute_m3_train"]["step1"] == "recompute" and f["mid_recompute_m3_train"]["pool"] is None
    assert f["mid_stored_m3_train"]["step1"] == "combine" and f["mid_stored_m3_train"]["pool"] == "kernel"   # N % 128 != 0
    assert f["mid_pool_m3_train"]["pool"] == "tiles" and f["mid_eval_m3_eval"]["pool"] == "kernel"
    assert f["mid_stored_m0_train"]["fwd"] == fp32_7 and not f["mid_stored_m0_train"]["mat"]
    assert f["mid_stored_m1_train"]["fwd"] == ("fp32",) * 4 + ("s3",) * 3
    assert f["mid_stored_m1_train"]["fusion"] == ("fp32", "s3") and not f["mid_stored_m1_train"]["recompute_ok"]
    # P >= 8192: every launch but conv1's (K = 4 or 8) on the split cores, held wgrads with the apply pass
    big = dict(fwd=("fp32",) + ("h2",) * 6, fusion=("h2tr+apply", "h2"), conv_dgrad=("fp32", "fp32", "h2", "h2", "h2"),
               conv_wgrad=("fp32",) + ("h2tr+apply",) * 4, mat=True, recompute_ok=True)
    for cid, pool, step1 in (("big_recompute_m3_train", None, "recompute"), ("big_both_m3_train", "kernel", "combine"),
                             ("big_c6_m3_train", None, "recompute"), ("big_pool_m3_train", "tiles", "combine")):
        assert f[cid] == dict(big, pool=pool, step1=step1), cid
    assert f["big_both_m1_train"] == dict(fwd=("fp32",) + ("s3",) * 6, fusion=("s3", "s3"), pool="kernel", step1="combine",
                                          conv_dgrad=("fp32", "fp32", "s3", "s3", "s3"),
                                          conv_wgrad=("fp32",) + ("s3",) * 4, mat=False, recompute_ok=False)
    assert K.BY_ID["big_pool_m3_train"].P == 8192 and K.BY_ID["big_both_m3_train"].P == 8197


# ------------------------------------------------------------------------------------------ plumbing
def _p(t):
    return C.c_void_p(0 if t is None or t.numel() == 0 else t.data_ptr())


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _guarded(rows, width, dtype=torch.float32):
    """A (rows, width) view of sentinels (NaN; INT_SENTINEL for integers) with GUARD sentinel rows on either side;
    returns (view, whole)."""
    fill = float("nan") if dtype.is_floating_point else INT_SENTINEL
    whole = torch.full((rows + 2 * GUARD, width), fill, dtype=dtype, device="cuda")
    return whole[GUARD:GUARD + rows], whole


def _untouched(t):
    return bool(torch.isnan(t).all()) if t.dtype.is_floating_point else bool((t == INT_SENTINEL).all())


def _guards_intact(whole):
    return _untouched(whole[:GUARD]) and _untouched(whole[-GUARD:])


def _vec(width):
    v, whole = _guarded(1, width)
    return v[0], whole


def _same(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def _np(t):
    return t.detach().cpu().numpy()


def _worst(a, b):
    """max that keeps a NaN (Python's max drops one in its second argument)."""
    return float("nan") if a != a or b != b else max(a, b)


@pytest.fixture()
def lib_mode():
    """The library, with a setter for the GEMM mode that is undone afterwards."""
    from pointnet_refine_amd import _lib
    lib = _lib.lib()
    old = lib.prh_get_gemm_mode()

    def set_mode(m):
        assert lib.prh_set_gemm_mode(m) == 0
        return lib
    yield set_mode
    lib.prh_set_gemm_mode(old)


class Encoder:
    """Device copies of an input set and the two entry points around them."""

    def __init__(self, lib, key):
        self.lib, self.key = lib, key
        self.C, self.B, self.N, self.od, self.training = key
        self.P, self.cat = self.B * self.N, sum(E.CONV_WIDTHS) + self.od
        prm, running, ctx, d_fused, d_gfeat = K.inputs(key)
        dev = lambda a: torch.from_numpy(np.array(a)).cuda()
        layers = prm["conv"] + [prm["fusion"]]
        p2 = [None] * 28                                  # ops.ENC_PARAM_ORDER
        for l in range(5):
            p2[2 * l], p2[2 * l + 1] = dev(layers[l]["w"]), dev(layers[l]["b"])
            p2[10 + 2 * l], p2[11 + 2 * l] = dev(layers[l]["gamma"]), dev(layers[l]["beta"])
        p2[20:24] = [dev(prm["fusion"][k]) for k in ("w", "b", "gamma", "beta")]
        p2[24:28] = [dev(prm["w1"]).reshape(64, 1), dev(prm["b1"]), dev(prm["w2"]), dev(prm["b2"])]
        self.p2 = p2
        self.bufs0 = [t for l, (rm, rv) in enumerate(running)
                      for t in (dev(rm), dev(rv), torch.tensor(K.NBT0 + l, dtype=torch.int64, device="cuda"))]
        self.ctx = dev(ctx).reshape(self.B, self.N, self.C)
        self.d_fused, self.d_gfeat = dev(d_fused), dev(d_gfeat)

    def workspace_bytes(self, backward, B=None, N=None):
        return int(self.lib.prh_encoder_workspace_bytes(B or self.B, N or self.N, self.C, self.od, backward))

    def forward(self, pooled=True, store_gate=True, op_amax=False, ws=None, ws_bytes=None, B=None, N=None,
                training=None, in_channel=None):
        from pointnet_refine_amd import _lib as L, ops
        B, N = B or self.B, N or self.N
        P, od, cat = B * N, self.od, self.cat
        training = self.training if training is None else training
        bufs = [t.clone() for t in self.bufs0]
        out = dict(P=P, B=B, N=N, training=training, bufs=bufs, gate=None, gfeat=None, argmax=None, op_amax=None)
        wholes = []
        for k, w in (("z_cat", cat), ("z_fus", od), ("fused", od)) + ((("gate", od),) if store_gate else ()):
            out[k], whole = _guarded(P, w)
            wholes.append(whole)
        for k in COEF:
            out[k], whole = _vec(cat + od)
            wholes.append(whole)
        if op_amax:
            out["op_amax"], whole = _vec(8)
            wholes.append(whole)
        if pooled:
            out["gfeat"], whole = _guarded(B, 2 * od)
            out["argmax"], whole_i = _guarded(B, od, torch.int32)
            wholes += [whole, whole_i]
        out["wholes"] = wholes
        prm = ops._enc_params_struct(self.p2, bufs, self.C if in_channel is None else in_channel)
        sv = L.EncoderSaved(_p(out["z_cat"]), _p(out["z_fus"]), _p(out["gate"]), _p(out["scale"]), _p(out["shift"]),
                            _p(out["mean"]), _p(out["rstd"]), _p(out["argmax"]), _p(out["op_amax"]))
        if ws is None:
            ws = torch.empty(self.workspace_bytes(0, B, N), dtype=torch.uint8, device="cuda")
        nbytes = ws.numel() if ws_bytes is None else ws_bytes
        ctx = self.ctx if (B, N) == (self.B, self.N) else self.ctx[:B, :N].contiguous()
        rc = self.lib.prh_encoder_forward(C.byref(prm), _p(ctx), B, N, training, K.MOMENTUM, K.EPS, _p(out["fused"]),
                                          _p(out["gfeat"]), C.byref(sv), _p(ws), nbytes, 0, _stream())
        torch.cuda.synchronize()
        return rc, out

    def backward(self, fw, d_fused=True, d_gfeat=True, recompute=0, scratch=0, null=(), want_dctx=True, ws=None,
                 ws_bytes=None, with_argmax=True):
        """null: names of gradient pointers passed as NULL ("conv2.dw", "fusion.dgamma", "d_gate_w1", ...)."""
        from pointnet_refine_amd import _lib as L, ops
        P, od = self.P, self.od
        wholes = []
        d, d_whole = _guarded(P, od)
        d.copy_(self.d_fused)
        gate, gate_whole = _guarded(P, od)                # recompute: uninitialised scratch for dG
        if not recompute:
            gate.copy_(fw["gate"])
        sv = L.EncoderSaved(_p(fw["z_cat"]), _p(fw["z_fus"]), _p(gate), _p(fw["scale"]), _p(fw["shift"]), _p(fw["mean"]),
                            _p(fw["rstd"]), _p(fw["argmax"] if with_argmax else None), _p(fw["op_amax"]), int(recompute))
        got = dict(conv=[], d_fused=d, d_fused_whole=d_whole, dG=gate, gate_whole=gate_whole, gate_before=gate.clone())
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
        if ws is None:
            ws = torch.empty(self.workspace_bytes(2 if scratch else 1), dtype=torch.uint8, device="cuda")
        nbytes = ws.numel() if ws_bytes is None else ws_bytes
        rc = self.lib.prh_encoder_backward(C.byref(prm), _p(self.ctx), self.B, self.N, fw["training"],
                                           _p(d if d_fused else None), _p(self.d_gfeat if d_gfeat else None),
                                           int(scratch), C.byref(sv), C.byref(gr), _p(got["d_ctx"] if want_dctx else None),
                                           _p(ws), nbytes, 0, _stream())
        torch.cuda.synchronize()
        return rc, got

    def outputs_untouched(self, fw=None, bw=None):
        """No launch wrote anything: every output still holds its sentinels and the statistics their initial values."""
        ok = True
        if fw is not None:
            ok = ok and all(_untouched(w) for w in fw["wholes"])
            ok = ok and all(torch.equal(a, b) for a, b in zip(fw["bufs"], self.bufs0))
        if bw is not None:
            ok = ok and all(_untouched(w) for w in bw["wholes"]) and _same(bw["d_fused"], self.d_fused)
            ok = ok and _same(bw["dG"], bw["gate_before"])
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


def _check_forward(en, fw, ref, pooled, stored):
    """Error / gate of every forward quantity (<= 1 passes), the device's masks and arg-max, mask flips and arg-max
    differences against the reference's own, and the list of hard failures."""
    od, cat, B, N, bad = en.od, en.cat, en.B, en.N, []
    prm, running, ctx, _, _ = K.inputs(en.key)
    if not all(_guards_intact(w) for w in fw["wholes"]):
        bad.append("forward wrote into a guard row")
    z_cat, z_fus = _np(fw["z_cat"]), _np(fw["z_fus"])
    co = {k: _np(fw[k]) for k in COEF}
    dm = E.device_masks(ctx, prm, z_cat, z_fus, co["scale"], co["shift"], od, _np(fw["argmax"]) if pooled else None)
    q = dict(z=0.0, y=0.0, mean=0.0, rstd=0.0, scale=0.0, shift=0.0, running_mean=0.0, running_var=0.0)
    widths = list(E.CONV_WIDTHS) + [od, od]
    off = np.concatenate([[0], np.cumsum(widths)])
    flips = 0
    for l, r in enumerate(ref["conv"] + [ref["fus"]]):
        s = slice(off[l], off[l + 1])
        z = z_cat[:, s] if l < 5 else z_fus
        q["z"] = _worst(q["z"], K.fwd_ratio(r["z"], z))
        for k in COEF:
            q[k] = _worst(q[k], K.fwd_ratio(r[k], co[k][s]))
        rm, rv, nbt = fw["bufs"][3 * l:3 * l + 3]
        if fw["training"]:
            q["running_mean"] = _worst(q["running_mean"], K.fwd_ratio(r["running_mean"], _np(rm)))
            q["running_var"] = _worst(q["running_var"], K.fwd_ratio(r["running_var"], _np(rv)))
        elif not (_same(rm, en.bufs0[3 * l]) and _same(rv, en.bufs0[3 * l + 1])):
            bad.append(f"eval mode touched the running statistics of layer {l}")
        want = K.NBT0 + l + (1 if fw["training"] else 0)
        if int(nbt) != want:
            bad.append(f"num_batches_tracked of layer {l}: {int(nbt)}, expected {want}")
        # the post-BN value every consumer rebuilds from the saved z, scale and shift
        y_dev = z.astype(np.float64) * co["scale"][s].astype(np.float64) + co["shift"][s].astype(np.float64)
        q["y"] = _worst(q["y"], K.fwd_ratio(r["y"], y_dev))
        flip = (dm["conv"][l] if l < 5 else dm["fus"]) != r["mask"]
        flips += int(flip.sum())
        if (flip & (np.abs(r["y"]) > S.band(r["y"], K.GATE_FWD, 1.0))).any():
            bad.append(f"layer {l}: a ReLU mask differs from the reference's outside the band")
    if not np.array_equal(dm["hidden"], ref["gate"]["hmask"]):
        bad.append("the gate hidden mask is a function of the fp32 inputs alone and differs")
    fused = _np(fw["fused"])
    q["fused"] = K.fwd_ratio(ref["F"], fused)
    if stored:
        q["gate"] = K.fwd_ratio(ref["gate"]["m"], _np(fw["gate"]))
    argdiff = 0
    if pooled:
        gfeat, arg = _np(fw["gfeat"]), _np(fw["argmax"]).astype(np.int64)
        q["gfeat"] = K.fwd_ratio(ref["gfeat"], gfeat)
        Fb = fused.reshape(B, N, od)
        if not np.array_equal(arg, np.argmax(Fb, axis=1)):
            bad.append("argmax is not the first arg-max of the device's own fused")
        elif not np.array_equal(gfeat[:, :od].view(np.int32), np.take_along_axis(Fb, arg[:, None, :], axis=1)[:, 0].view(np.int32)):
            bad.append("gfeat's max half is not fused at argmax, bit for bit")
        else:
            Fr = ref["F"].reshape(B, N, od)
            short = ref["gfeat"][:, :od] - np.take_along_axis(Fr, arg[:, None, :], axis=1)[:, 0]
            if short.max() > 2.0 * S.band(ref["F"], K.GATE_FWD, 1.0):
                bad.append("the reference's F at the device's arg-max is not within twice the band of its maximum")
        if arg[:, K.DEAD].any():
            bad.append("the dead channel's arg-max is not point 0")
        argdiff = int((arg != ref["argmax"]).sum())
    return q, dm, flips, argdiff, bad


def _reference_backward(en, fw, dm, d_fused=True, d_gfeat=True):
    prm, running, ctx, dF, dG = K.inputs(en.key)
    co = {k: _np(fw[k]) for k in COEF}
    conv, fus = E.records_from_saved(_np(fw["z_cat"]), _np(fw["z_fus"]), co["scale"], co["shift"], co["mean"], co["rstd"],
                                     en.od, dm)
    return E.backward(dF if d_fused else None, dG if d_gfeat else None, ctx, en.B, en.N, prm, conv, fus,
                      fw["training"], dm)


def _verdict(tag, q, bad, limits={}):
    print(tag, " ".join(f"{k}={v:.3f}" for k, v in q.items()), "|", "; ".join(bad) if bad else "ok")
    over = {k: round(v, 3) for k, v in q.items() if not v <= limits.get(k, 1.0)}
    assert not bad and not over, (tag, bad, over)


def _limits():
    return {k: v / K.GATE_GRAD for k, v in K.OWN_GATES.items()}


# ------------------------------------------------------------------------------------------ the cases
@pytest.mark.parametrize("case", K.CASES, ids=[c.id for c in K.CASES])
def test_encoder_forward_and_backward_against_fp64(lib_mode, case):
    lib = lib_mode(case.mode)
    if case.recompute:
        assert lib.prh_encoder_gate_recompute(case.B, case.N, case.C, case.od, 0) == 1
    en = Encoder(lib, case.inputs)
    ref = K.reference_forward(case.inputs)
    rc, fw = en.forward(pooled=case.pooled, store_gate=not case.recompute, op_amax=case.op_amax)
    assert rc == 0, lib.prh_last_error()
    qf, dm, flips, argdiff, bad = _check_forward(en, fw, ref, case.pooled, not case.recompute)
    ref_bw = _reference_backward(en, fw, dm, case.d_fused, case.d_gfeat)
    keep = {k: fw[k].clone() for k in ("z_cat", "z_fus") + COEF + (("op_amax",) if case.op_amax else ())}
    rc, bw = en.backward(fw, case.d_fused, case.d_gfeat, case.recompute, case.scratch)
    assert rc == 0, lib.prh_last_error()
    qb = K.quantities(ref_bw, _grads_np(bw), fw["training"])
    if not all(_guards_intact(w) for w in bw["wholes"] + [bw["d_fused_whole"], bw["gate_whole"]]):
        bad.append("backward wrote into a guard row")
    prm, running, ctx, _, d_gfeat = K.inputs(case.inputs)
    if not (all(_same(keep[k], fw[k]) for k in keep) and np.array_equal(_np(en.ctx).reshape(-1, case.C), ctx)
            and np.array_equal(_np(en.d_gfeat), d_gfeat)):
        bad.append("the backward changed one of its inputs")
    if not case.scratch and not _same(bw["d_fused"], en.d_fused):
        bad.append("d_fused changed without d_fused_scratch")
    if not fw["training"] and not all(np.abs(_np(g["db"])).max() > 0 for g in bw["conv"] + [bw["fusion"]]):
        bad.append("an eval-mode db is zero")
    _verdict(f"ENC {case.id} mode={case.mode} flips={flips} argdiff={argdiff}", {**qf, **qb}, bad, _limits())


# ------------------------------------------------------------------------------------------ contract edges
MID = K.BY_ID["mid_recompute_m3_train"]
SMALL = K.BY_ID["small_m3_train"]


def test_recomputed_and_stored_gate_give_the_same_bits_on_these_inputs(lib_mode):
    """mid_recompute's path (gate = NULL, gate_recompute, d_fused as scratch) against the stored gate with d_fused read
    only, the same outputs requested: one set of bits, which ties the fp64 result of either case to both paths."""
    lib = lib_mode(3)
    en = Encoder(lib, MID.inputs)
    rc, fw_s = en.forward(pooled=False, store_gate=True, op_amax=True)
    assert rc == 0, lib.prh_last_error()
    rc, fw_n = en.forward(pooled=False, store_gate=False, op_amax=True)
    assert rc == 0, lib.prh_last_error()
    for k in ("z_cat", "z_fus", "fused", "op_amax") + COEF:
        assert _same(fw_s[k], fw_n[k]), k
    rc, a = en.backward(fw_s, d_gfeat=False, recompute=0, scratch=0)
    assert rc == 0, lib.prh_last_error()
    rc, b = en.backward(fw_n, d_gfeat=False, recompute=1, scratch=1)
    assert rc == 0, lib.prh_last_error()
    ta, tb = _grad_tensors(a), _grad_tensors(b)
    assert all(_same(ta[k], tb[k]) for k in ta), [k for k in ta if not _same(ta[k], tb[k])]
    assert _same(a["dG"], b["dG"]) and not any(torch.isnan(v).any() for v in tb.values())
    assert _guards_intact(b["d_fused_whole"]) and all(_guards_intact(w) for w in a["wholes"] + b["wholes"])


def test_null_gradient_pointers_and_null_d_ctx_leave_the_rest_bit_equal(lib_mode):
    lib = lib_mode(3)
    en = Encoder(lib, SMALL.inputs)
    rc, fw = en.forward()
    assert rc == 0, lib.prh_last_error()
    rc, full = en.backward(fw)
    assert rc == 0, lib.prh_last_error()
    null = ("conv1.db", "conv2.dw", "conv3.dbeta", "fusion.dw", "fusion.dgamma", "d_gate_w1", "d_gate_b1")
    rc, part = en.backward(fw, null=null)
    assert rc == 0, lib.prh_last_error()
    tf, tp = _grad_tensors(full), _grad_tensors(part)
    assert all(torch.isnan(tp[k]).all() for k in null)
    assert all(_same(tf[k], tp[k]) for k in tf if k not in null), [k for k in tf if k not in null and not _same(tf[k], tp[k])]
    rc, no_dx = en.backward(fw, want_dctx=False)
    assert rc == 0, lib.prh_last_error()
    tn = _grad_tensors(no_dx, skip=("d_ctx",))
    assert torch.isnan(no_dx["d_ctx"]).all() and all(_same(tf[k], tn[k]) for k in tn)
    assert all(_guards_intact(w) for w in part["wholes"] + no_dx["wholes"])


def test_bad_arguments_are_refused_without_a_launch(lib_mode):
    lib = lib_mode(3)
    en = Encoder(lib, SMALL.inputs)
    rc, fw = en.forward()
    assert rc == 0, lib.prh_last_error()
    # d_fused_scratch together with d_gfeat
    rc, bw = en.backward(fw, scratch=1)
    assert rc == PRH_ERR_ARG and b"d_fused_scratch" in lib.prh_last_error() and en.outputs_untouched(bw=bw)
    # gate_recompute where prh_encoder_gate_recompute() says no: P = 129 is below the grid floor of the split cores
    assert lib.prh_encoder_gate_recompute(en.B, en.N, en.C, en.od, 0) == 0
    rc, bw = en.backward(fw, d_gfeat=False, recompute=1, scratch=1)
    assert rc == PRH_ERR_ARG and b"gate_recompute" in lib.prh_last_error() and en.outputs_untouched(bw=bw)
    # d_gfeat without argmax
    rc, bw = en.backward(fw, with_argmax=False)
    assert rc == PRH_ERR_ARG and b"argmax" in lib.prh_last_error() and en.outputs_untouched(bw=bw)
    # training with one point
    rc, one = en.forward(B=1, N=1, training=1)
    assert rc == PRH_ERR_ARG and b"more than 1 value" in lib.prh_last_error() and en.outputs_untouched(fw=one)
    # three input channels: no intensity
    rc, c3 = en.forward(in_channel=3)
    assert rc == PRH_ERR_ARG and b"at least 4 channels" in lib.prh_last_error() and en.outputs_untouched(fw=c3)


@pytest.mark.parametrize("mode", [0, 3])
def test_a_missing_or_short_workspace_is_refused(lib_mode, mode):
    """Present, and no smaller than prh_encoder_workspace_bytes reports - else PRH_ERR_WORKSPACE before the device is
    touched.  (The entry points used to test the carve alone: a NULL workspace with a non-zero size passed it, every
    carved pointer NULL, and so did one up to 256 bytes short.)"""
    lib = lib_mode(mode)
    en = Encoder(lib, SMALL.inputs)
    none = torch.empty(0, dtype=torch.uint8, device="cuda")
    n = en.workspace_bytes(0)
    ws = torch.empty(n, dtype=torch.uint8, device="cuda")
    rc, fw = en.forward(ws=ws, ws_bytes=n - 1)
    assert rc == PRH_ERR_WORKSPACE and en.outputs_untouched(fw=fw), lib.prh_last_error()
    rc, fw = en.forward(ws=none, ws_bytes=n)
    assert rc == PRH_ERR_WORKSPACE and en.outputs_untouched(fw=fw), lib.prh_last_error()
    rc, fw = en.forward(ws=ws)
    assert rc == 0, lib.prh_last_error()
    for scratch, kw in ((0, {}), (1, dict(d_gfeat=False))):
        n = en.workspace_bytes(2 if scratch else 1)
        ws = torch.empty(n, dtype=torch.uint8, device="cuda")
        rc, bw = en.backward(fw, scratch=scratch, ws=ws, ws_bytes=n - 1, **kw)
        assert rc == PRH_ERR_WORKSPACE and en.outputs_untouched(bw=bw), lib.prh_last_error()
        rc, bw = en.backward(fw, scratch=scratch, ws=none, ws_bytes=n, **kw)
        assert rc == PRH_ERR_WORKSPACE and en.outputs_untouched(bw=bw), lib.prh_last_error()
        rc, bw = en.backward(fw, scratch=scratch, ws=ws, **kw)
        assert rc == 0 and not any(torch.isnan(v).any() for v in _grad_tensors(bw).values()), lib.prh_last_error()


def test_the_bf16_pair_refuses_a_missing_or_short_workspace(lib_mode):
    """The same defect and the same rule on prh_encoder_forward_bf16 / prh_encoder_backward_bf16; their numerics are
    pinned in tests/test_encoder16_abi_gpu.py (fp64 with the storage roundings of the bf16 contract), and
    tests/test_bf16_gpu.py asks whether bf16 is precise enough."""
    from pointnet_refine_amd import _lib as L, ops
    lib = lib_mode(4)
    en = Encoder(lib, SMALL.inputs)
    P, od, cat, B, N = en.P, en.od, en.cat, en.B, en.N
    BF16_NAN = 0x7FC0
    h = lambda rows, w: torch.full((rows, w), BF16_NAN, dtype=torch.int16, device="cuda")
    z_cat, z_fus, gate, fused, d_fused = h(P, cat), h(P, od), h(P, od), h(P, od), h(P, od)
    coef = torch.full((4, cat + od), float("nan"), device="cuda")
    gfeat = torch.full((B, 2 * od), float("nan"), device="cuda")
    argmax = torch.full((B, od), INT_SENTINEL, dtype=torch.int32, device="cuda")
    bufs = [t.clone() for t in en.bufs0]
    sv = L.EncoderSavedBf16(_p(z_cat), _p(z_fus), _p(gate), _p(coef[0]), _p(coef[1]), _p(coef[2]), _p(coef[3]), _p(argmax))
    grads = [torch.full(t.shape, float("nan"), device="cuda") for t in en.p2]
    gr = L.EncoderGrads()
    for k in range(5):
        gr.conv[k] = L.BnLayerGrad(_p(grads[2 * k]), _p(grads[2 * k + 1]), _p(grads[10 + 2 * k]), _p(grads[11 + 2 * k]))
    gr.fusion = L.BnLayerGrad(_p(grads[20]), _p(grads[21]), _p(grads[22]), _p(grads[23]))
    gr.d_gate_w1, gr.d_gate_b1, gr.d_gate_w2, gr.d_gate_b2 = (_p(grads[i]) for i in (24, 25, 26, 27))
    d_ctx = torch.full((P, en.C), float("nan"), device="cuda")
    none = torch.empty(0, dtype=torch.uint8, device="cuda")

    def untouched():
        torch.cuda.synchronize()
        return (all(bool((t == BF16_NAN).all()) for t in (z_cat, z_fus, gate, fused, d_fused)) and _untouched(coef)
                and _untouched(gfeat) and _untouched(argmax) and _untouched(d_ctx) and all(_untouched(g) for g in grads)
                and all(torch.equal(a, b) for a, b in zip(bufs, en.bufs0)))
    n = int(lib.prh_encoder_bf16_workspace_bytes(B, N, en.C, od, 0))
    ws = torch.empty(n, dtype=torch.uint8, device="cuda")
    for w, nbytes in ((ws, n - 1), (none, n)):
        prm = ops._enc_params_struct(en.p2, bufs, en.C)
        rc = lib.prh_encoder_forward_bf16(C.byref(prm), _p(en.ctx), B, N, 1, K.MOMENTUM, K.EPS, _p(fused), _p(gfeat),
                                          C.byref(sv), _p(w), nbytes, 0, _stream())
        assert rc == PRH_ERR_WORKSPACE and untouched(), lib.prh_last_error()
    n = int(lib.prh_encoder_bf16_workspace_bytes(B, N, en.C, od, 1))
    ws = torch.empty(n, dtype=torch.uint8, device="cuda")
    for w, nbytes in ((ws, n - 1), (none, n)):
        prm = ops._enc_params_struct(en.p2, None, en.C)
        rc = lib.prh_encoder_backward_bf16(C.byref(prm), _p(en.ctx), B, N, 1, _p(d_fused), _p(en.d_gfeat), C.byref(sv),
                                           C.byref(gr), _p(d_ctx), _p(w), nbytes, 0, _stream())
        assert rc == PRH_ERR_WORKSPACE and untouched(), lib.prh_last_error()
