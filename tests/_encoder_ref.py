"""fp64 numpy reference of the multi-scale point encoder (pointnet_refine_amd/model.py:39-62), forward and backward.

    feat_l = relu(bn_l(conv_l(.)))                 l = 1..5
    zf     = cat(feat_1..5) @ Wf^T + bf ;  yf = bn_f(zf)
    u      = relu(inten*w1 + b1) ;  a = u @ W2^T + b2 ;  m = 0.5 + 0.5*sigmoid(a)
    F      = relu(yf) * m
    gfeat  = [max_n F | mean_n F]   (first arg-max)

Built on tests/_stack_ref.py: conv1..5 are a five-layer stack with a ReLU behind every layer, the fusion layer is a
one-layer stack over the concat.  `prm` is dict(conv=[5 layer dicts], fusion=layer dict, w1 [64], b1 [64],
w2 [out_dim, 64], b2 [out_dim]); `running` is six (running_mean, running_var) pairs, conv1..5 then fusion.

Every ReLU is where(mask, y, 0) and the max-pool's gradient goes to a given index, so the backward takes its five
conv masks, the fusion mask, the gate-hidden mask and the arg-max as inputs (default: the forward's own).  With the
device's masks (device_masks, hidden_mask) and the device's arg-max the encoder is linear algebra, BatchNorm and one
sigmoid, and two evaluations differ by arithmetic error alone.  The gate m is always computed here, in fp64, from ctx
and the weights: it depends on nothing a device saved.  No torch, no GPU.

The bf16-storage contract (prh_encoder_forward_bf16 / prh_encoder_backward_bf16) is the SAME statement with the
storage hook of tests/_stack_ref.py: store=None is the fp32 contract above, store=_stack_ref.BF16 rounds to nearest
even wherever that contract stores or feeds a 16-bit value (pack_bf16x2 is v_cvt_pk_bf16_f32).  The rounding points,
each read in the kernel named (csrc/prh_b16.hpp, csrc/prh_gemm.hpp, csrc/prh_lib.hip):
  forward
    conv1, C <= 8      z1 = store(b + W x), fp32 operands, fmaf chain in channel order (conv_in_b16_kernel): store_first = 0
    conv1, C > 8       x (cast_b16_kernel) and W (prep_weights_b16_kernel) stored, rows zero-padded to a multiple of 8
                       channels; z1 = store(acc + b) (gemm_nt_b16_kernel: bf16_round(acc + b) in front of the epilogue)
    conv2..5, fusion   A = store(relu(fmaf(z_prev, scale, shift))) (store_tile of gemm_nt_b16_kernel), W = store(W),
                       z = store(acc + b)
    statistics         of the STORED z (epi_col_stats runs behind the rounding; conv_in_b16_kernel sums its rounded
                       outputs); rstd, scale, shift and the running statistics as in the fp32 contract
    gate               u = store(relu(fmaf(inten, w1, b1))), W2 = store(W2), m = 0.5 + 0.5*sigmoid(acc + b2) in fp32;
                       the saved gate is store(m); fused = store(relu(fmaf(zf, s, t)) * m) with the UNROUNDED m
                       (EPI_GATE of nt_epilogue_vec: ev_store packs m and v separately)
    pooling            max and first arg-max over the stored `fused`, mean = fp32 sum / N (pool_b16_kernel; the
                       F_POOL epilogue rounds v before it compares and sums)
  backward
    combine step       d = dF (bf16 as supplied) + d_gfeat's mean term / N + its max term at the arg-max;
                       dy_f = store(pre > 0 ? d*m : 0) with m the SAVED (stored) gate, sig = 2m - 1,
                       dG = store(d * r * 0.5*sig*(1 - sig)); the BatchNorm sums are taken from the stored dy_f
                       (combine_bwd_b16_kernel, combine_bwd_b16v_kernel)
    BN apply           dz = store(fmaf(ka, dy, fmaf(kb, z, kc))) in place (bn_bwd_apply_b16_kernel); db is NOT the sum
                       of the stored dz: bn_bwd_finalize_kernel forms it from the two sums, i.e. of the unrounded dz
    wgrads             operands are the stored dz and the stored prologue activations (store_tile of
                       gemm_tn_b16_kernel); slabs fp32, summed in fp64
    fusion dgrad       its block of dy_cat = store(mask(dz_f . store(W)))  (EPI_DGRAD, C16)
    conv dgrads        accumulate: new = store(mask(old + dz . store(W))), old read back from its bf16 buffer (F_ACCUM);
                       the sums for the layer below are taken from the stored result
    conv1              dW for C <= 8 from the fp32 ctx rows (conv_in_wgrad_b16_kernel), for C > 8 from the stored,
                       padded x with the pad columns dropped; d_ctx = dz_1 . store(W1) in fp32 for every C (the
                       weight image of the dgrad is prep_weights_b16_kernel's)
    gate part          the stored dG is the operand of both GEMMs, u = store(relu(fmaf(inten, w1, b1))) the other
                       operand of dW2; dU = mask(dG . store(W2)) and everything behind it is fp32
"""
import numpy as np

import _stack_ref as S

MUTATIONS = ("mean_grad_over_P", "argmax_last_tie", "skip_grad_dropped", "gate_hidden_unmasked",
             "dctx_intensity_dropped", "fusion_mask_from_gated", "gate_grad_without_relu_factor")
# deliberate mistakes of the bf16-storage contract alone (tests/test_encoder16_ref_cpu.py): an accumulating dgrad
# that overwrites its block of dy_cat, BatchNorm sums of the fusion layer taken from the unrounded dy_f, and the
# padded conv1 wgrad (C > 8) copied out with the padded leading dimension ignored, so that pad columns stay
MUTATIONS_STORED = ("dgrad_overwrites", "sums_from_unrounded_dy", "pad_column_kept")
CONV_WIDTHS = (64, 128, 256, 512)


def _f64(a):
    return np.asarray(a, dtype=np.float64)


def hidden_mask(ctx2d, prm):
    """The gate-hidden ReLU as a kernel takes it, fmaf(inten, w1, b1) > 0: the product of two fp32 numbers is exact in
    fp64 and the sum's sign survives its one rounding (the argument of _stack_ref.device_masks)."""
    return _f64(ctx2d[:, 3])[:, None] * _f64(prm["w1"]) + _f64(prm["b1"]) > 0


def gate(ctx2d, prm, hmask=None, store=None):
    """u, a, sig and m = 0.5 + 0.5*sig of the intensity gate; hmask stands in for the hidden layer's own u > 0.
    With a store, u and W2 are the stored operands; m stays unrounded (the saved gate is store(m))."""
    pre = _f64(ctx2d[:, 3])[:, None] * _f64(prm["w1"]) + _f64(prm["b1"])
    own = pre > 0
    u = S.stored(store, np.where(own if hmask is None else hmask, pre, 0.0))
    a = S.result(store, u @ S.stored(store, _f64(prm["w2"])).T + _f64(prm["b2"]))
    sig = 1.0 / (1.0 + np.exp(-a))
    return dict(pre=pre, hmask=own, u=u, a=a, sig=sig, m=S.result(store, 0.5 + 0.5 * sig))


def pool(F, B, N, mutation=None):
    """[max | mean] over the N points of each of the B segments and the arg-max: the first one, as torch.max."""
    Fb = F.reshape(B, N, -1)
    if mutation == "argmax_last_tie":
        arg = N - 1 - np.argmax(Fb[:, ::-1], axis=1)
    else:
        arg = np.argmax(Fb, axis=1)
    gmax = np.take_along_axis(Fb, arg[:, None, :], axis=1)[:, 0]
    return np.concatenate([gmax, Fb.mean(axis=1)], axis=1), arg.astype(np.int64)


def store_first(C):
    """Whether conv1's operands are stored: C <= 8 runs on the fp32 context rows (conv_in_fp32_ok)."""
    return int(C > 8)


def forward(ctx2d, B, N, prm, training, momentum, eps, running, mutation=None, store=None):
    """ctx2d [B*N, C].  conv: the five records of _stack_ref.forward; fus: the fusion layer's record (out = relu(yf));
    gate: gate(); F [P, out_dim]; gfeat [B, 2*out_dim]; argmax [B, out_dim].  With a store also gate_stored, the
    saved gate."""
    conv = S.forward(ctx2d, prm["conv"], training, momentum, eps, 1, running[:5], store=store,
                     store_first=store_first(np.shape(ctx2d)[1]))
    cat = np.concatenate([r["out"] for r in conv], axis=1)
    fus = S.forward(cat, [prm["fusion"]], training, momentum, eps, 1, running[5:], store=store)[0]
    g = gate(ctx2d, prm, store=store)
    F = S.stored(store, fus["out"] * g["m"])
    gfeat, arg = pool(F, B, N, mutation)
    gfeat = S.result(store, gfeat)
    return dict(conv=conv, fus=fus, gate=g, F=F, gfeat=gfeat, argmax=arg, gate_stored=S.stored(store, g["m"]))


def own_masks(fw):
    return dict(conv=[r["mask"] for r in fw["conv"]], fus=fw["fus"]["mask"], hidden=fw["gate"]["hmask"],
                argmax=fw["argmax"])


def records_from_saved(z_cat, z_fus, scale, shift, mean, rstd, out_dim, masks):
    """(conv records, fusion record) of a saved forward: z_cat [P, cat], z_fus [P, out_dim] and the coefficient
    vectors of length cat + out_dim, conv1..5 first."""
    widths = list(CONV_WIDTHS) + [out_dim]
    cat = sum(widths)
    conv = S.records_from_saved(z_cat, scale[:cat], shift[:cat], mean[:cat], rstd[:cat], widths, 1, masks["conv"])
    fus = S.records_from_saved(z_fus, scale[cat:], shift[cat:], mean[cat:], rstd[cat:], [out_dim], 1, [masks["fus"]])[0]
    return conv, fus


def device_masks(ctx2d, prm, z_cat, z_fus, scale, shift, out_dim, argmax):
    """The masks of a saved forward, exactly as its kernels took them, and its recorded arg-max."""
    widths = list(CONV_WIDTHS) + [out_dim]
    cat = sum(widths)
    return dict(conv=S.device_masks(z_cat, scale[:cat], shift[:cat], widths),
                fus=S.device_masks(z_fus, scale[cat:], shift[cat:], [out_dim])[0],
                hidden=hidden_mask(ctx2d, prm), argmax=None if argmax is None else np.asarray(argmax, np.int64))


def pooled_terms(d_fused, d_gfeat, B, N, od, argmax, mutation=None):
    """dF_total = dF + d_mean / N + [n == argmax] * d_max, [P, od], and the sum of the magnitudes of its terms."""
    dF = np.zeros((B, N, od)) if d_fused is None else _f64(d_fused).reshape(B, N, od).copy()
    mag = np.abs(dF)
    if d_gfeat is not None:
        dg = _f64(d_gfeat)
        dF += dg[:, None, od:] / (B * N if mutation == "mean_grad_over_P" else N)
        mag += np.abs(dg[:, None, od:]) / N
        bi, ci = np.meshgrid(np.arange(B), np.arange(od), indexing="ij")
        dF[bi, argmax, ci] += dg[:, :od]
        mag[bi, argmax, ci] += np.abs(dg[:, :od])
    return dF.reshape(B * N, od), mag.reshape(B * N, od)


def backward(d_fused, d_gfeat, ctx2d, B, N, prm, conv, fus, training, masks, mutation=None, m_dtype=None, store=None,
             m_saved=None, coeff_dtype=None):
    """Gradients of sum(d_fused * F) + sum(d_gfeat * gfeat) (either may be None) from the records of a forward.
    Returns d_ctx [P, C], conv: five dicts(dw, db, dgamma, dbeta, dz), fusion: one such dict, d_gate_w1, d_gate_b1,
    d_gate_w2, d_gate_b2, and dG (= da, for the tests' scales).
    m_dtype: round the gate m to this type and form sig = 2m - 1 from the rounded value, nothing else: what storing
    the gate in fp32 costs (1 - sig cancels where the sigmoid saturates).
    store: the storage hook (module docstring); then m_saved, the saved gate [P, out_dim], is m and sig = 2m - 1.
    coeff_dtype: as _stack_ref.backward, for all six layers."""
    P = B * N
    od = fus["z"].shape[1]
    x = _f64(ctx2d)
    sf = store_first(x.shape[1])
    g = gate(ctx2d, prm, masks["hidden"], store)
    m = g["m"]
    if m_saved is not None:
        m = _f64(m_saved)
        sig = 2.0 * m - 1.0
    elif m_dtype is not None:
        m = _f64(m.astype(m_dtype))
        sig = 2.0 * m - 1.0
    else:
        sig = g["sig"]
    dF = S.result(store, pooled_terms(d_fused, d_gfeat, B, N, od, masks["argmax"], mutation)[0])
    fmask = masks["fus"]
    if mutation == "fusion_mask_from_gated":      # F > 0 taken after multiplying by the gate's pre-activation, not by m
        fmask = fus["y"] * g["a"] > 0
    r = np.where(fmask, fus["y"], 0.0)
    da = S.stored(store, dF * (1.0 if mutation == "gate_grad_without_relu_factor" else r) * 0.5 * sig * (1.0 - sig))
    # fusion layer over the concat: the mask is applied by the one-layer stack's relu_last
    cat_out = np.concatenate([c["out"] for c in conv], axis=1)
    dyf = dF * m
    if store is not None:
        dyf = store(np.where(fmask, dyf, 0.0))
    unrounded = np.where(fmask, dF * m, 0.0) if mutation == "sums_from_unrounded_dy" else None
    g_cat, gf = S.backward(dyf, cat_out, [prm["fusion"]], [fus], training, 1, [fmask], coeff_dtype=coeff_dtype,
                           store=store, dy_stats=unrounded)
    # conv5..1: each block of the concat gradient is ADDED to what the next conv's dgrad sends back, then masked
    off = np.concatenate([[0], np.cumsum([c["z"].shape[1] for c in conv])])
    grads = [None] * 5
    carry = 0.0
    for l in range(4, -1, -1):
        blk = g_cat[:, off[l]:off[l + 1]]
        if store is not None:       # the fusion dgrad's block as its bf16 buffer holds it
            blk = store(np.where(masks["conv"][l], blk, 0.0))
        if mutation in ("skip_grad_dropped", "dgrad_overwrites") and l < 4:
            blk = 0.0
        gl = S.stored(store, np.where(masks["conv"][l], blk + carry, 0.0))
        h = conv[l - 1]["out"] if l > 0 else x
        carry, one = S.backward(gl, h, [prm["conv"][l]], [conv[l]], training, 0, [None], coeff_dtype=coeff_dtype,
                                store=store, store_first=sf if l == 0 else 1)
        grads[l] = one[0]
    if mutation == "pad_column_kept" and sf:      # [cout, c0p] copied out as if its rows were C long
        cout, C = grads[0]["dw"].shape
        padded = np.zeros((cout, -(-C // 8) * 8))
        padded[:, :C] = grads[0]["dw"]
        grads[0]["dw"] = padded.reshape(-1)[:cout * C].reshape(cout, C)
    d_ctx = carry.copy()
    # intensity gate
    du = S.result(store, da @ S.stored(store, _f64(prm["w2"])))
    if mutation != "gate_hidden_unmasked":
        du = np.where(masks["hidden"], du, 0.0)
    if mutation != "dctx_intensity_dropped":
        d_ctx[:, 3] += du @ _f64(prm["w1"])
    d_ctx = S.result(store, d_ctx)
    return dict(d_ctx=d_ctx, conv=grads, fusion=gf[0], d_gate_w2=S.result(store, da.T @ g["u"]),
                d_gate_b2=S.result(store, da.sum(axis=0)), d_gate_w1=S.result(store, (du * x[:, 3:4]).sum(axis=0)),
                d_gate_b1=S.result(store, du.sum(axis=0)), dG=da, dU=du)


def band_shares(fw, tol, floor=1.0):
    """(share over the five conv layers and the fusion layer, share of the gate hidden layer) of the values feeding
    a ReLU with |y| <= tol * max(floor, max|y| of their layer)."""
    main = S.band_share(fw["conv"] + [fw["fus"]], tol, 1, floor)
    pre = fw["gate"]["pre"]
    return main, float((np.abs(pre) <= S.band(pre, tol, floor)).sum()) / pre.size
