"""tests/_stack_ref.py, the fp64 reference of the shared-MLP stack, checked on the CPU:
(a) against stock torch.nn in double (Linear + BatchNorm1d + ReLU, differentiated by autograd);
(b) forcing the reference's own masks reproduces it bit for bit;
(c) the inputs of every case of tests/test_mlp_stack_gpu.py keep the share of post-BN values that sit within the
    forward gate of a ReLU's kink at or below 1e-3, so that mask flips stay a rarity the GPU test can bound;
(d) the same inputs tell the contract from each of four deliberate mistakes (_stack_ref.MUTATIONS, the reference's
    counterparts of wrong kernels): every mistake moves at least one output past the GPU test's gate.
"""
import numpy as np
import pytest
import torch

import _stack_cases as K
import _stack_ref as R

MOMENTUM, EPS = K.MOMENTUM, K.EPS


def _torch_stack(layers, running, relu_last, training):
    mods = []
    for l, (ly, rn) in enumerate(zip(layers, running)):
        cout, cin = ly["w"].shape
        lin = torch.nn.Linear(cin, cout).double()
        bn = torch.nn.BatchNorm1d(cout, eps=EPS, momentum=MOMENTUM).double()
        with torch.no_grad():
            lin.weight.copy_(torch.from_numpy(np.asarray(ly["w"], np.float64)))
            lin.bias.copy_(torch.from_numpy(np.asarray(ly["b"], np.float64)))
            bn.weight.copy_(torch.from_numpy(np.asarray(ly["gamma"], np.float64)))
            bn.bias.copy_(torch.from_numpy(np.asarray(ly["beta"], np.float64)))
            bn.running_mean.copy_(torch.from_numpy(np.asarray(rn[0], np.float64)))
            bn.running_var.copy_(torch.from_numpy(np.asarray(rn[1], np.float64)))
        mods += [lin, bn]
        if R.has_relu(l, len(layers), relu_last):
            mods.append(torch.nn.ReLU())
    m = torch.nn.Sequential(*mods)
    return m.train() if training else m.eval()


def _small_inputs(cin, P, seed):
    widths = (cin, 8, 12, 4)
    layers, running = K._seeded_layers(widths, seed)
    g = np.random.default_rng([seed, P, cin])
    return layers, running, g.standard_normal((P, cin)), g.standard_normal((P, widths[-1]))


@pytest.mark.parametrize("P", [2, 77])
@pytest.mark.parametrize("cin", [3, 6])
@pytest.mark.parametrize("relu_last", [0, 1])
@pytest.mark.parametrize("training", [1, 0])
def test_reference_equals_torch_double_and_forced_own_masks_are_a_no_op(training, relu_last, cin, P):
    layers, running, x, dy = _small_inputs(cin, P, seed=5)
    recs = R.forward(x, layers, training, MOMENTUM, EPS, relu_last, running)
    masks = [r["mask"] for r in recs]
    dx, grads = R.backward(dy, x, layers, recs, training, relu_last, masks)

    m = _torch_stack(layers, running, relu_last, training)
    xt = torch.from_numpy(x).requires_grad_(True)
    out = m(xt)
    out.backward(torch.from_numpy(dy))
    tol = 1e-10
    assert R.rel_l2(out.detach().numpy(), recs[-1]["out"]) < tol
    assert R.rel_l2(xt.grad.numpy(), dx) < tol
    lins = [mod for mod in m if isinstance(mod, torch.nn.Linear)]
    bns = [mod for mod in m if isinstance(mod, torch.nn.BatchNorm1d)]
    for l, (lin, bn) in enumerate(zip(lins, bns)):
        assert R.rel_l2(bn.running_mean.numpy(), recs[l]["running_mean"]) < tol, l
        assert R.rel_l2(bn.running_var.numpy(), recs[l]["running_var"]) < tol, l
        assert int(bn.num_batches_tracked) == (1 if training else 0)
        assert R.rel_l2(lin.weight.grad.numpy(), grads[l]["dw"]) < tol, l
        assert R.rel_l2(bn.weight.grad.numpy(), grads[l]["dgamma"]) < tol, l
        assert R.rel_l2(bn.bias.grad.numpy(), grads[l]["dbeta"]) < tol, l
        if training:      # analytically zero: measured against the size of what cancels
            assert np.abs(lin.bias.grad.numpy() - grads[l]["db"]).max() <= tol * np.abs(grads[l]["dz"]).sum(axis=0).max()
        else:
            assert R.rel_l2(lin.bias.grad.numpy(), grads[l]["db"]) < tol and np.abs(grads[l]["db"]).max() > 0
    if not training:
        for l in range(len(layers)):
            assert np.array_equal(recs[l]["running_mean"], np.asarray(running[l][0], np.float64))
            assert np.array_equal(recs[l]["running_var"], np.asarray(running[l][1], np.float64))

    # (b) the reference's own masks, forced: the same bits, forward and backward
    again = R.forward(x, layers, training, MOMENTUM, EPS, relu_last, running, masks=masks)
    for r0, r1 in zip(recs, again):
        for k in r0:
            assert np.array_equal(r0[k], r1[k]), k
    saved = R.records_from_saved(np.concatenate([r["z"] for r in recs], axis=1), *[
        np.concatenate([r[k] for r in recs]) for k in ("scale", "shift", "mean", "rstd")],
        [ly["w"].shape[0] for ly in layers], relu_last, masks)
    dx2, grads2 = R.backward(dy, x, layers, saved, training, relu_last, masks)
    assert np.array_equal(dx, dx2)
    for g0, g1 in zip(grads, grads2):
        for k in g0:
            assert np.array_equal(g0[k], g1[k]), k
    # device_masks on exact fp64 "saved" values is the own mask
    dm = R.device_masks(np.concatenate([r["z"] for r in recs], axis=1), np.concatenate([r["scale"] for r in recs]),
                        np.concatenate([r["shift"] for r in recs]), [ly["w"].shape[0] for ly in layers])
    assert all(np.array_equal(a, b) for a, b in zip(dm, masks))


INPUT_SETS = sorted({c.inputs for c in K.CASES}, key=str)


@pytest.mark.parametrize("key", INPUT_SETS, ids=[str(k) for k in INPUT_SETS])
def test_band_share_of_every_gpu_input_set(key):
    widths, P, training, relu_last, weights = key
    recs = K.reference_forward(key)
    share = R.band_share(recs, K.GATE_FWD, relu_last, floor=1.0)
    print(f"band share {share:.3e}  {key}")
    assert share <= 1e-3


def test_gamma_variant_separates_adjacent_dz_maxima():
    """The gamma x 2^8 weights: the largest |dz| of two adjacent layers differ by at least 2^10, so a split-fp16
    operand scale read from the neighbour's header costs ten bits or overflows."""
    for P in (8192, 8197):
        key = K.Case(K.GAMMA_STACK, P, weights="gamma256").inputs
        layers, running, x, dy = K.inputs(key)
        recs = K.reference_forward(key)
        _, grads = R.backward(dy, x, layers, recs, 1, 0, [r["mask"] for r in recs])
        mx = [float(np.abs(g["dz"]).max()) for g in grads]
        print(f"P={P} max|dz| per layer {mx}")
        assert mx[K.GAMMA_LAYER] / mx[K.GAMMA_LAYER + 1] >= 2.0 ** 10


def test_two_rows_put_the_gradients_beyond_fp32_coefficients():
    """Why the P = 2 case of the GPU test has gates of its own for dx, dw and db.  With two rows BatchNorm's backward
    cancels but for eps: dz = gamma * rstd * eps / (var + eps) * (...), here 1e-6 and less of its terms.  The kernels
    form dz = ca*dy + cb*z + cc from three fp32 vectors; rounding those three vectors ALONE, everything else exact,
    already moves dx, dw and db past 1e-5 - by orders of magnitude at P = 2 and not at all at P = 77."""
    worst = {}
    for P in (2, 77):
        key = K.Case(K.POINT_MLP, P, weights="point_mlp").inputs
        layers, running, x, dy = K.inputs(key)
        recs = K.reference_forward(key)
        masks = [r["mask"] for r in recs]
        dx0, g0 = R.backward(dy, x, layers, recs, 1, 0, masks)
        dx1, g1 = R.backward(dy, x, layers, recs, 1, 0, masks, coeff_dtype=np.float32)
        worst[P] = dict(dx=K.grad_ratio(dx0, dx1), dw=max(K.grad_ratio(a["dw"], b["dw"]) for a, b in zip(g0, g1)),
                        db=max(K.db_ratio(a["db"], b["db"], a["dz"]) for a, b in zip(g0, g1)))
        print(f"P={P}: fp32 coefficients alone, error / gate {worst[P]}")
    assert min(worst[2].values()) > 1.0 and max(worst[77].values()) < 0.1
    assert worst[2]["dx"] > 10.0 and worst[2]["dw"] > 10.0


def _outputs(key, mutation=None):
    widths, P, training, relu_last, weights = key
    layers, running, x, dy = K.inputs(key)
    recs = R.forward(x, layers, training, MOMENTUM, EPS, relu_last, running, mutation=mutation)
    masks = [r["mask"] for r in recs]
    dx, grads = R.backward(dy, x, layers, recs, training, relu_last, masks, mutation=mutation)
    return recs, dx, grads


@pytest.mark.parametrize("P", [77, 8197])
@pytest.mark.parametrize("mutation", R.MUTATIONS)
def test_inputs_detect_each_mutation_of_the_reference(mutation, P):
    relu_last = 1 if mutation == "relu_last_ignored" else 0
    key = K.Case(K.POINT_MLP, P, relu_last=relu_last, weights="point_mlp").inputs
    good, dx0, g0 = _outputs(key)
    bad, dx1, g1 = _outputs(key, mutation)
    worst = {"dx": K.grad_ratio(dx0, dx1)}
    for l in range(len(g0)):
        worst[f"running_var{l}"] = K.fwd_ratio(good[l]["running_var"], bad[l]["running_var"])
        for k in ("dw", "dgamma", "dbeta"):
            worst[f"{k}{l}"] = K.grad_ratio(g0[l][k], g1[l][k])
        worst[f"db{l}"] = K.db_ratio(g0[l]["db"], g1[l]["db"], g0[l]["dz"])
    top = max(worst, key=worst.get)
    print(f"{mutation} P={P}: largest error / gate {worst[top]:.3g} in {top}")
    assert worst[top] > 1.0
