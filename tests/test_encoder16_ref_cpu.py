"""The bf16-storage statement of tests/_encoder_ref.py (the `store` hook) and the cases and gates of
tests/test_encoder16_abi_gpu.py, checked on the CPU:
(a) store=None, the fp32 contract, is untouched by the hook: on every input set of tests/_encoder_cases.py it gives the
    bits of a Store whose rounding is the identity, which walks through every hook point - the hook's roundings are the
    ONLY difference between the two contracts (there is one forward and one backward, not two);
(b) _stack_ref.bf16 is round-to-nearest-even to 8 significant bits: the bits of torch's fp32 -> bf16 cast, ties included;
    the store=bf16 forward holds representable values and takes its statistics from them;
(c) each case of tests/_encoder16_cases.py selects the launch paths it is named for;
(d) the gates of the backward chain follow from what one fp32 evaluation of the chain costs against the fp64 one
    (_encoder16_cases.FIGURES, GATES), measured here from the reference alone;
(e) teeth: every deliberate mistake of _encoder_ref.MUTATIONS and MUTATIONS_STORED, applied to the store=bf16 chain,
    moves the quantity it names by at least 10 times that quantity's gate.  None falls short.
"""
import numpy as np
import pytest
import torch

import _encoder16_cases as K16
import _encoder_cases as K
import _encoder_ref as E
import _stack_ref as S


def _flat(o, pre=""):
    if isinstance(o, dict):
        for k, v in o.items():
            yield from _flat(v, f"{pre}.{k}")
    elif isinstance(o, (list, tuple)):
        for i, v in enumerate(o):
            yield from _flat(v, f"{pre}[{i}]")
    elif o is not None:
        yield pre, np.asarray(o)


# ------------------------------------------------------------------------------------------ (a) store=None
@pytest.mark.parametrize("key", K.INPUT_SETS, ids=[str(k) for k in K.INPUT_SETS])
def test_no_store_is_the_fp32_contract_bit_for_bit(key):
    C, B, N, od, training = key
    prm, running, ctx, d_fused, d_gfeat = K.inputs(key)
    same = S.Store(rounding=lambda a: a)
    plain = K.reference_forward(key)
    hooked = E.forward(ctx, B, N, prm, training, K.MOMENTUM, K.EPS, running, store=same)
    a, b = dict(_flat(plain)), dict(_flat(hooked))
    assert a.keys() == b.keys() and all(np.array_equal(a[k], b[k]) for k in a), [k for k in a if not np.array_equal(a[k], b[k])]
    assert plain["gate_stored"] is plain["gate"]["m"]
    masks = E.own_masks(plain)
    g0 = E.backward(d_fused, d_gfeat, ctx, B, N, prm, plain["conv"], plain["fus"], training, masks)
    g1 = E.backward(d_fused, d_gfeat, ctx, B, N, prm, plain["conv"], plain["fus"], training, masks, store=same)
    a, b = dict(_flat(g0)), dict(_flat(g1))
    assert a.keys() == b.keys() and all(np.array_equal(a[k], b[k]) for k in a), [k for k in a if not np.array_equal(a[k], b[k])]


# ------------------------------------------------------------------------------------------ (b) the rounding
def test_bf16_rounding_is_torchs_cast_ties_to_even():
    g = np.random.default_rng(5)
    x = np.concatenate([g.standard_normal(200000) * np.exp(g.uniform(-30, 30, 200000)),
                        [0.0, -0.0, 1.0, 1.00390625, 1.01171875, -1.00390625, 3.0e-30, 255.5, 256.5 * 2.0 ** 60]]).astype(np.float32)
    want = torch.from_numpy(x).to(torch.bfloat16).to(torch.float64).numpy()
    got = S.bf16(x)
    assert np.array_equal(got, want)
    assert S.bf16(1.00390625) == 1.0 and S.bf16(1.01171875) == 1.015625          # ties: to the even neighbour
    assert np.array_equal(K16.from_bits16(K16.bits16(got[:1000])), got[:1000])
    assert np.array_equal(K16.bits16(got), torch.from_numpy(x).to(torch.bfloat16).view(torch.int16).numpy().view(np.uint16))
    # one fp32 evaluation: through float32 first, as a kernel's registers
    y = g.standard_normal(1000) * 1e-3
    assert np.array_equal(S.BF16_VIA_F32(y), S.bf16(y.astype(np.float32)))


@pytest.mark.parametrize("key", [K16.BY_ID["small_train"].inputs, K16.BY_ID["c12_train"].inputs,
                                 K16.BY_ID["tails_eval"].inputs], ids=["small", "c12", "tails_eval"])
def test_the_stored_forward_holds_bf16_values_and_their_statistics(key):
    C, B, N, od, training = key
    prm, running, ctx, _, _ = K.inputs(key)
    fw = E.forward(ctx, B, N, prm, training, K.MOMENTUM, K.EPS, running, store=S.BF16)
    rep = lambda a: np.array_equal(S.bf16(a), a)
    for l, r in enumerate(fw["conv"] + [fw["fus"]]):
        assert rep(r["z"]), l
        if training:
            assert np.array_equal(r["mean"], r["z"].mean(axis=0)), l
            assert np.allclose(r["rstd"], 1.0 / np.sqrt(r["z"].var(axis=0) + K.EPS), rtol=1e-12), l
    assert rep(fw["F"]) and rep(fw["gate_stored"]) and not rep(fw["gate"]["m"]) and rep(fw["gate"]["u"])
    # fused is the product with the UNROUNDED m, rounded once
    assert np.array_equal(fw["F"], S.bf16(fw["fus"]["out"] * fw["gate"]["m"]))
    assert np.array_equal(fw["gfeat"][:, :od], fw["F"].reshape(B, N, od).max(axis=1))
    assert not fw["F"][:, K.DEAD].any() and not fw["argmax"][:, K.DEAD].any()
    # conv1: fp32 operands up to 8 channels, stored operands (x and W) beyond
    x, w, b = (np.asarray(a, np.float64) for a in (ctx, prm["conv"][0]["w"], prm["conv"][0]["b"]))
    z1 = S.bf16(S.bf16(x) @ S.bf16(w).T + b) if C > 8 else S.bf16(x @ w.T + b)
    assert np.array_equal(fw["conv"][0]["z"], z1)
    # and against the fp32 contract the stored forward is bf16-close, nothing more: the hook rounds, it does not rewrite
    ref = E.forward(ctx, B, N, prm, training, K.MOMENTUM, K.EPS, running)
    assert S.rel_l2(ref["F"], fw["F"]) < 3e-2 and S.rel_l2(ref["fus"]["z"], fw["fus"]["z"]) < 3e-2


# ------------------------------------------------------------------------------------------ (c) selection
def test_the_cases_select_the_launch_paths_they_are_named_for():
    """csrc/prh_lib.hip's rules for the two bf16 entry points restated (tests/_encoder16_cases.py), so that a moved
    threshold does not silently turn these cases into repeats of one another."""
    f = {c.id: K16.families(c) for c in K16.CASES}
    assert all(v["lds_ok"] and not v["pacing"] for v in f.values())
    every = ("fusion", "conv5", "conv4", "conv3", "conv2", "gate")
    all_dma = {k: "dma" for k in every}
    for cid in ("small_train", "small_eval"):       # one ragged row tile, segment ends inside it, 128 threads per row
        assert f[cid] == dict(conv1="valu", partial_k=(), col_tail=(64, 128, 1984), dgrad=all_dma, d_ctx="staged_fp32", combine=128,
                              pool=("kernel",), row_tiles=1, stat_tiles=2, splits={k: 1 for k in every}, pacing=False,
                              lds_ok=True), cid
    for cid in ("tails_train", "tails_eval"):
        c, v = K16.BY_ID[cid], f[cid]
        assert c.C == 6 and c.cat == 1096 and c.cat % 64 == 8 and v["conv1"] == "valu" and v["partial_k"] == ("fusion",)
        assert v["col_tail"] == (64, 128, 136, 1096) and v["combine"] == "scalar" and v["d_ctx"] is None
        assert v["dgrad"] == dict(all_dma, fusion="staged", conv5="staged", gate="staged") and v["pool"] == ("kernel",)
    v = f["c12_train"]
    assert v["conv1"] == "padded" and v["combine"] == 32 and v["d_ctx"] == "staged_fp32" and v["splits"]["conv1"] == 1
    assert K16.BY_ID["c12_train"].C % 8 == 4 and K16.BY_ID["c12_train"].C % 4 == 0      # pad columns exist; d_ctx allowed
    v = f["od512_train"]
    assert v["combine"] == 64 and v["pool"] == ("tiles", 1) and v["conv1"] == "valu"
    v = f["mid_train"]
    assert K16.BY_ID["mid_train"].P == 2049 and v["row_tiles"] == 9 and v["stat_tiles"] == 17 and v["pool"] == ("kernel",)
    assert v["splits"] == dict(fusion=5, conv5=5, conv4=5, conv3=5, conv2=5, gate=5) and v["combine"] == 128
    for cid, pool in (("mid_pool_gfeat_only_train", ("tiles", 2)), ("mid_pool_fused_only_train", None),
                      ("mid_pool_both_train", ("tiles", 2))):
        assert f[cid]["pool"] == pool and f[cid]["row_tiles"] == 8 and f[cid]["splits"]["fusion"] == 4, cid
    c = K16.BY_ID
    assert (c["mid_pool_gfeat_only_train"].d_fused, c["mid_pool_gfeat_only_train"].d_gfeat) == (0, 1)
    assert (c["mid_pool_fused_only_train"].d_fused, c["mid_pool_fused_only_train"].d_gfeat) == (1, 0)
    v = f["od2048_train"]
    assert v["combine"] == 256 and K16.BY_ID["od2048_train"].cat == 3008 and v["pool"] == ("tiles", 1)
    assert K16.nt_b16_lds(3008, True) == 156160 and K16.nt_b16_lds(3968, True) == 160 * 1024 < K16.nt_b16_lds(3969, True)
    # the three thread shapes of the vector combine kernel and the scalar one are all here
    assert {v["combine"] for v in f.values()} == {32, 64, 128, 256, "scalar"}


# ------------------------------------------------------------------------------------------ (d) gates
def test_the_gates_follow_from_what_one_fp32_evaluation_costs():
    """The store=bf16 chain twice per training input set on one saved forward - in fp64, and with every GEMM and
    elementwise result through float32 in front of the same roundings: the largest error per quantity is the figure of
    _encoder16_cases.FIGURES (written there rounded up by 2 to 10 %), and the gate is max(GATE_GRAD, 4 * figure)."""
    worst = {}
    for key in K16.TRAINING_SETS:
        q = K16.quantities(K16.chain(key, S.BF16), K16.chain(key, S.BF16_VIA_F32), 1)
        for k, v in q.items():
            worst[k] = max(worst.get(k, 0.0), v * K.GATE_GRAD)
    print("one fp32 evaluation against fp64, largest rel error per quantity:")
    print(" ".join(f"{k}={v:.3e}" for k, v in worst.items()))
    assert worst.keys() == K16.FIGURES.keys() == K16.GATES.keys()
    for k, v in worst.items():
        fig = K16.FIGURES[k][0]
        assert fig / 1.25 <= v <= fig, (k, v, fig)
        assert K16.GATES[k] == max(K.GATE_GRAD, 4.0 * fig) and K16.limits()[k] == K16.GATES[k] / K.GATE_GRAD
    assert min(K16.GATES.values()) == K.GATE_GRAD and max(K16.GATES.values()) < 2.1e-2
    # eval mode: db = scale * dbeta takes dbeta's gate; one fp32 evaluation costs it no more than dbeta's figure
    for key in (k for k in K16.INPUT_SETS if not k[4]):
        q = K16.quantities(K16.chain(key, S.BF16), K16.chain(key, S.BF16_VIA_F32), 0)
        for k in (k for k in q if k.endswith(".db")):
            print(f"eval {key} {k}: {q[k] * K.GATE_GRAD:.3e}, dbeta's figure {K16.FIGURES[k[:-2] + 'dbeta'][0]:.1e}")
            assert q[k] * K.GATE_GRAD <= K16.FIGURES[k[:-2] + "dbeta"][0], (key, k)
            assert K16.limits(0)[k] == K16.limits(1)[k[:-2] + "dbeta"]


# ------------------------------------------------------------------------------------------ (e) teeth
# mutation -> (the case whose inputs show it, the compared quantity that moves by at least 10 of its gates there)
DETECTS = {
    "mean_grad_over_P": ("small_train", "fusion.dbeta"),
    "argmax_last_tie": ("small_train", "argmax"),      # compared exactly; a tie's gradient is zero either way
    "skip_grad_dropped": ("small_train", "conv4.dw"),
    "gate_hidden_unmasked": ("small_train", "d_gate_b1"),
    "dctx_intensity_dropped": ("c12_train", "d_ctx3"),      # the gate's share of d_ctx[:, 3] is 4 % at C = 4, 27 % here
    "fusion_mask_from_gated": ("small_train", "fusion.dw"),
    "gate_grad_without_relu_factor": ("small_train", "d_gate_w2"),
    "dgrad_overwrites": ("small_train", "conv4.dw"),
    "sums_from_unrounded_dy": ("small_train", "fusion.dgamma"),
    "pad_column_kept": ("c12_train", "conv1.dw"),
}


@pytest.mark.parametrize("mutation", E.MUTATIONS + E.MUTATIONS_STORED)
def test_the_stored_chain_detects_each_mutation(mutation):
    case_id, quantity = DETECTS[mutation]
    case = K16.BY_ID[case_id]
    key = case.inputs
    fw = K16.saved_forward(key)
    good = K16.chain(key, S.BF16)
    if mutation == "argmax_last_tie":
        _, arg = E.pool(fw["F"], case.B, case.N, mutation)
        assert (arg != fw["argmax"]).any() and (arg[:, K.DEAD] == case.N - 1).all()
        return
    bad = K16.chain(key, S.BF16, mutation=mutation)
    lim = K16.limits()
    r = {k: v / lim[k] for k, v in K16.quantities(good, bad, case.training).items()}
    top = max(r, key=r.get)
    print(f"{mutation} {case_id}: {quantity} moves by {r[quantity]:.3g} of its gates (largest: {top}, {r[top]:.3g})")
    assert r[quantity] >= 10.0
