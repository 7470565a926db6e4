"""tests/_encoder_ref.py, the fp64 reference of the encoder, checked on the CPU:
(a) against oracle/linerefine_oracle.py's encoder_forward in torch double, differentiated by autograd, and forcing
    the reference's own masks (through records_from_saved / device_masks on its exact values) is a no-op;
(b) the inputs of tests/test_encoder_abi_gpu.py tell the contract from each deliberate mistake of
    _encoder_ref.MUTATIONS by more than 100 times the GPU test's gate of the quantity named in DETECTS;
(c) every input set keeps the share of values that feed a ReLU within the forward gate of its kink at or below 1e-3
    (five conv layers and the fusion layer together; the gate hidden layer on its own);
(d) what storing the gate m in fp32 and forming sig = 2m - 1 from it costs the gate's gradients: the figures behind
    _encoder_cases.OWN_GATES.
"""
import numpy as np
import pytest
import torch

import _encoder_cases as K
import _encoder_ref as E
import _stack_ref as S

TOL = 1e-10
SIZES = {"small": (3, 43, 1024), "tails": (5, 7, 132)}


def _oracle_params(prm, running):
    t = lambda a: torch.from_numpy(np.asarray(a, np.float64).copy())
    p = {}
    names = [(f"conv{k}", f"bn{k}") for k in range(1, 6)] + [("fusion.0", "fusion.1")]
    for (conv, bn), ly, (rm, rv) in zip(names, prm["conv"] + [prm["fusion"]], running):
        p[f"{conv}.weight"], p[f"{conv}.bias"] = t(ly["w"])[:, :, None], t(ly["b"])
        p[f"{bn}.weight"], p[f"{bn}.bias"] = t(ly["gamma"]), t(ly["beta"])
        p[f"{bn}.running_mean"], p[f"{bn}.running_var"] = t(rm), t(rv)
        p[f"{bn}.num_batches_tracked"] = torch.tensor(0)
    p["intensity_gate.0.weight"], p["intensity_gate.0.bias"] = t(prm["w1"])[:, None, None], t(prm["b1"])
    p["intensity_gate.2.weight"], p["intensity_gate.2.bias"] = t(prm["w2"])[:, :, None], t(prm["b2"])
    for k, v in p.items():
        if v.is_floating_point() and "running" not in k:
            v.requires_grad_(True)
    return p, names


@pytest.mark.parametrize("size", list(SIZES))
@pytest.mark.parametrize("C", [4, 6])
@pytest.mark.parametrize("training", [1, 0])
def test_reference_equals_the_oracle_in_double_and_forced_own_masks_are_a_no_op(monkeypatch, training, C, size):
    from oracle import linerefine_oracle as O
    monkeypatch.setattr(O, "BN_EPS", K.EPS)
    monkeypatch.setattr(O, "BN_MOMENTUM", K.MOMENTUM)
    B, N, od = SIZES[size]
    prm, running, ctx, d_fused, d_gfeat = K.inputs((C, B, N, od, training))
    fw = E.forward(ctx, B, N, prm, training, K.MOMENTUM, K.EPS, running)
    masks = E.own_masks(fw)
    bw = E.backward(d_fused, d_gfeat, ctx, B, N, prm, fw["conv"], fw["fus"], training, masks)

    p, names = _oracle_params(prm, running)
    x = torch.from_numpy(ctx.astype(np.float64).reshape(B, N, C)).requires_grad_(True)
    stats = {}
    gfeat, fused = O.encoder_forward(p, x, training=bool(training), new_stats=stats)
    ((fused * torch.from_numpy(d_fused.astype(np.float64)).reshape(B, N, od)).sum() +
     (gfeat * torch.from_numpy(d_gfeat.astype(np.float64))).sum()).backward()
    assert S.rel_l2(fused.detach().numpy().reshape(B * N, od), fw["F"]) < TOL
    assert S.rel_l2(gfeat.detach().numpy(), fw["gfeat"]) < TOL
    assert np.array_equal(fused.detach().max(dim=1)[1].numpy(), fw["argmax"])
    assert not fw["F"][:, K.DEAD].any() and not fw["argmax"][:, K.DEAD].any()      # the dead channel: point 0
    assert S.rel_l2(x.grad.numpy().reshape(B * N, C), bw["d_ctx"]) < TOL
    recs = fw["conv"] + [fw["fus"]]
    for l, ((conv, bn), g) in enumerate(zip(names, bw["conv"] + [bw["fusion"]])):
        if training:
            assert S.rel_l2(stats[f"{bn}.running_mean"].numpy(), recs[l]["running_mean"]) < TOL, l
            assert S.rel_l2(stats[f"{bn}.running_var"].numpy(), recs[l]["running_var"]) < TOL, l
        else:
            assert not stats and np.array_equal(recs[l]["running_var"], np.asarray(running[l][1], np.float64))
        assert S.rel_l2(p[f"{conv}.weight"].grad.numpy()[:, :, 0], g["dw"]) < TOL, l
        assert S.rel_l2(p[f"{bn}.weight"].grad.numpy(), g["dgamma"]) < TOL, l
        assert S.rel_l2(p[f"{bn}.bias"].grad.numpy(), g["dbeta"]) < TOL, l
        db = p[f"{conv}.bias"].grad.numpy()
        if training:      # analytically zero: measured against the size of what cancels
            assert np.abs(db - g["db"]).max() <= TOL * np.abs(g["dz"]).sum(axis=0).max(), l
        else:
            assert S.rel_l2(db, g["db"]) < TOL and np.abs(g["db"]).max() > 0, l
    assert S.rel_l2(p["intensity_gate.0.weight"].grad.numpy().reshape(-1), bw["d_gate_w1"]) < TOL
    assert S.rel_l2(p["intensity_gate.0.bias"].grad.numpy(), bw["d_gate_b1"]) < TOL
    assert S.rel_l2(p["intensity_gate.2.weight"].grad.numpy()[:, :, 0], bw["d_gate_w2"]) < TOL
    assert S.rel_l2(p["intensity_gate.2.bias"].grad.numpy(), bw["d_gate_b2"]) < TOL

    # the reference's own saved forward and its own masks, the way the GPU test rebuilds them: the same bits
    cat = lambda k: np.concatenate([r[k] for r in recs])
    z_cat = np.concatenate([r["z"] for r in fw["conv"]], axis=1)
    dm = E.device_masks(ctx, prm, z_cat, fw["fus"]["z"], cat("scale"), cat("shift"), od, fw["argmax"])
    assert all(np.array_equal(a, b) for a, b in zip(dm["conv"], masks["conv"]))
    assert np.array_equal(dm["fus"], masks["fus"]) and np.array_equal(dm["hidden"], masks["hidden"])
    conv, fus = E.records_from_saved(z_cat, fw["fus"]["z"], cat("scale"), cat("shift"), cat("mean"), cat("rstd"), od, dm)
    again = E.backward(d_fused, d_gfeat, ctx, B, N, prm, conv, fus, training, dm)
    assert np.array_equal(again["d_ctx"], bw["d_ctx"]) and np.array_equal(again["d_gate_w1"], bw["d_gate_w1"])
    for g0, g1 in zip(bw["conv"] + [bw["fusion"]], again["conv"] + [again["fusion"]]):
        assert all(np.array_equal(g0[k], g1[k]) for k in g0)


# ------------------------------------------------------------------------------------------ (b) mutations
# mutation -> (the case whose inputs show it, the compared quantity that moves by more than 100 gates there)
DETECTS = {
    "mean_grad_over_P": ("small_m3_train", "d_ctx"),
    "argmax_last_tie": ("small_m3_train", "argmax"),      # compared exactly; a tie's gradient is zero either way
    "skip_grad_dropped": ("small_m3_train", "conv1.dw"),
    "gate_hidden_unmasked": ("small_m3_train", "d_gate_b1"),
    "dctx_intensity_dropped": ("small_m3_train", "d_ctx3"),
    "fusion_mask_from_gated": ("small_m3_train", "fusion.dw"),
    "gate_grad_without_relu_factor": ("small_m3_train", "d_gate_w2"),
}


@pytest.mark.parametrize("mutation", E.MUTATIONS)
def test_inputs_detect_each_mutation_of_the_reference(mutation):
    case_id, quantity = DETECTS[mutation]
    case = K.BY_ID[case_id]
    prm, running, ctx, d_fused, d_gfeat = K.inputs(case.inputs)
    B, N, t = case.B, case.N, case.training
    fw = K.reference_forward(case.inputs)
    masks = E.own_masks(fw)
    good = E.backward(d_fused, d_gfeat, ctx, B, N, prm, fw["conv"], fw["fus"], t, masks)
    if mutation == "argmax_last_tie":
        _, arg = E.pool(fw["F"], B, N, mutation)
        moved = int((arg != fw["argmax"]).sum())
        print(f"{mutation} {case_id}: arg-max differs in {moved} (segment, channel) pairs, all {N - 1} in the dead one")
        assert moved > 0 and (arg[:, K.DEAD] == N - 1).all()
        bad = E.backward(d_fused, d_gfeat, ctx, B, N, prm, fw["conv"], fw["fus"], t, dict(masks, argmax=arg))
        assert max(K.quantities(good, bad, t).values()) == 0.0
        return
    bad = E.backward(d_fused, d_gfeat, ctx, B, N, prm, fw["conv"], fw["fus"], t, masks, mutation=mutation)
    q = K.quantities(good, bad, t)
    top = max(q, key=q.get)
    print(f"{mutation} {case_id}: {quantity} moves by {q[quantity]:.3g} gates (largest: {top}, {q[top]:.3g})")
    assert q[quantity] > 100.0


# ------------------------------------------------------------------------------------------ (c) band share
@pytest.mark.parametrize("key", K.INPUT_SETS, ids=[str(k) for k in K.INPUT_SETS])
def test_band_share_of_every_gpu_input_set(key):
    fw = K.reference_forward(key)
    main, hidden = E.band_shares(fw, K.GATE_FWD, floor=1.0)
    a = np.abs(fw["gate"]["a"]).max()
    print(f"band share conv+fusion {main:.3e} gate hidden {hidden:.3e} max|a| {a:.2f}  {key}")
    assert main <= 1e-3 and hidden <= 1e-3


# ------------------------------------------------------------------------------------------ (d) the fp32 stored gate
STORED_GATE_SETS = [c.inputs for c in (K.BY_ID["small_m3_train"], K.BY_ID["tails_m3_train"],
                                       K.BY_ID["mid_stored_m3_train"], K.BY_ID["big_both_m3_train"])]


@pytest.mark.parametrize("key", STORED_GATE_SETS, ids=[str(k) for k in STORED_GATE_SETS])
def test_what_the_fp32_stored_gate_costs(key):
    """m rounded to fp32 alone, sig = 2m - 1 from the rounded value, everything else in fp64: the rel-L2 cost on the
    gate's gradients and on d_ctx[:, 3].  Where the sigmoid saturates 1 - sig cancels (pre-activations reach 12 on the
    largest inputs: 1 - sig about 6e-6 against a spacing of 1.2e-7), but dG is small exactly there.  Measured: at most
    1.4e-7 (d_gate_w2, P = 8197), 1.3e-7 (d_gate_w1), 5.4e-8 (d_gate_b1), 4.3e-8 (d_gate_b2), 2.6e-8 (d_ctx[:, 3]).
    Below a tenth of the common gate no tensor can claim a gate of its own in the GPU test."""
    C, B, N, od, training = key
    prm, running, ctx, d_fused, d_gfeat = K.inputs(key)
    fw = K.reference_forward(key)
    masks = E.own_masks(fw)
    exact = E.backward(d_fused, d_gfeat, ctx, B, N, prm, fw["conv"], fw["fus"], training, masks)
    stored = E.backward(d_fused, d_gfeat, ctx, B, N, prm, fw["conv"], fw["fus"], training, masks, m_dtype=np.float32)
    cost = {k: S.rel_l2(exact[k], stored[k]) for k in ("d_gate_w2", "d_gate_b2", "d_gate_w1", "d_gate_b1")}
    cost["d_ctx3"] = S.rel_l2(exact["d_ctx"][:, 3], stored["d_ctx"][:, 3])
    print(f"fp32 stored gate, rel-L2 cost {key}: " + " ".join(f"{k}={v:.2e}" for k, v in cost.items()),
          f"max|a| {np.abs(fw['gate']['a']).max():.2f}")
    assert max(cost.values()) < 0.1 * K.GATE_GRAD
