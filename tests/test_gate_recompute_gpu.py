"""The encoder backward that computes the intensity gate again (saved.gate_recompute, EPI_GATE_BWD epilogue)
against the stored-gate path (combine_bwd_kernel) on the same inputs: every output bit for bit.

out_dim = 1024; the shapes are the smallest at which the second-generation split-fp16 core serves the gate
launch (>= 32 tiles of 256 x 256 and M >= 512, i.e. P > 1792): P = 2048 (aligned), P = 2000 (the last 64-row
block and the last row tile ragged), P = 2049 (a row tile of one row).  d_fused carries the cancelling
patterns of tests/_gate_recompute_ref.py, on which the contract's summation order differs from the cheaper
ones (tests/test_gate_recompute_cpu.py), so equal partial sums mean the same order.
"""
import ctypes as C

import numpy as np
import pytest
import torch

from _gate_recompute_ref import cancelling_matrix, contract_partials
from oracle import procedural as P

pytestmark = pytest.mark.gpu

OD, CIN = 1024, 4
CAT = 64 + 128 + 256 + 512 + OD
PAD = 64          # sentinel rows behind every [P, *] output
SHAPES = [(8, 256), (2, 1000), (3, 683)]


def _bits(t):
    return t.contiguous().view(torch.int32)


def _same(a, b):
    return a.shape == b.shape and torch.equal(_bits(a), _bits(b))


def _nan(*shape):
    return torch.full(shape, float("nan"), dtype=torch.float32, device="cuda")


@pytest.fixture(scope="module")
def lib():
    from pointnet_refine_amd import _lib
    l = _lib.lib()
    old = l.prh_get_gemm_mode()
    l.prh_set_gemm_mode(3)
    yield l
    l.prh_set_gemm_mode(old)


@pytest.fixture(scope="module")
def weights():
    from pointnet_refine_amd import ops
    sd = P.encoder_state_dict(CIN, OD, seed=3)
    p2 = []
    for k in ops.ENC_PARAM_ORDER:
        t = sd[k].float()
        p2.append((t.reshape(t.shape[0], -1) if t.dim() == 3 else t).contiguous().cuda())
    names = [f"bn{k}" for k in range(1, 6)] + ["fusion.1"]
    bufs = [sd[f"{n}.{s}"].clone().cuda() for n in names for s in ("running_mean", "running_var", "num_batches_tracked")]
    return p2, bufs


def _forward(lib, weights, B, N, store_gate, want_global=False):
    from pointnet_refine_amd import _lib as L, ops
    p2, bufs = weights
    bufs = [b.clone() for b in bufs]
    Pn = B * N
    x = P.synth_batch(B, N, CIN, 32, seed=11)[0].cuda().contiguous()
    z_cat, z_fus, fused = _nan(Pn + PAD, CAT), _nan(Pn + PAD, OD), _nan(Pn + PAD, OD)
    gate = _nan(Pn + PAD, OD) if store_gate else None
    coef = _nan(5, CAT + OD)
    gfeat = _nan(B, 2 * OD) if want_global else None
    argmax = torch.full((B, OD), -1, dtype=torch.int32, device="cuda") if want_global else None
    prm = ops._enc_params_struct(p2, bufs, CIN)
    sv = L.EncoderSaved(ops._p(z_cat), ops._p(z_fus), ops._p(gate), ops._p(coef[0]), ops._p(coef[1]), ops._p(coef[2]),
                        ops._p(coef[3]), ops._p(argmax), ops._p(coef[4]))
    ws = ops._ws(x.device, lib.prh_encoder_workspace_bytes(B, N, CIN, OD, 0))
    L.check(lib.prh_encoder_forward(C.byref(prm), ops._p(x), B, N, 1, 0.1, 1e-5, ops._p(fused), ops._p(gfeat),
                                    C.byref(sv), ops._p(ws), ws.numel(), x.device.index, ops._stream(x.device)),
            "prh_encoder_forward")
    torch.cuda.synchronize()
    return dict(x=x, z_cat=z_cat, z_fus=z_fus, fused=fused, gate=gate, coef=coef, bufs=bufs, gfeat=gfeat, argmax=argmax)


def _d_fused(Pn, seed):
    d = _nan(Pn + PAD, OD)
    d[:Pn] = torch.from_numpy(cancelling_matrix(Pn, OD, seed=seed)).cuda()
    return d


def _step1(lib, weights, fw, B, N, recompute, d_fused):
    """Step (1) of the backward on its own: (dy_f, dG, ws_a, ws_b), each with sentinel rows behind it."""
    from pointnet_refine_amd import ops
    p2, _ = weights
    Pn, nb = B * N, (B * N + 63) // 64
    d = d_fused.clone()
    gate = _nan(Pn + PAD, OD) if recompute else fw["gate"].clone()
    ws_a, ws_b = _nan(nb + 1, OD), _nan(nb + 1, OD)
    nbytes = lib.prh_test_gate_backward_workspace_bytes(OD)
    ws = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
    rc = lib.prh_test_gate_backward(ops._p(fw["x"]), B, N, CIN, OD, ops._p(p2[24]), ops._p(p2[25]), ops._p(p2[26]),
                                    ops._p(p2[27]), ops._p(fw["z_fus"]), ops._p(fw["coef"][0, CAT:]),
                                    ops._p(fw["coef"][1, CAT:]), ops._p(d), ops._p(gate), int(recompute), ops._p(ws_a),
                                    ops._p(ws_b), ops._p(ws), nbytes, 0, ops._stream(d.device))
    torch.cuda.synchronize()
    return rc, d, gate, ws_a, ws_b


def _backward(lib, weights, fw, B, N, recompute, d_fused, scratch=1, d_gfeat=None):
    """prh_encoder_backward; returns (rc, dict of every output)."""
    from pointnet_refine_amd import _lib as L, ops
    p2, _ = weights
    Pn = B * N
    d = d_fused.clone()
    gate = _nan(Pn + PAD, OD) if recompute else fw["gate"].clone()
    prm = ops._enc_params_struct(p2, None, CIN)
    sv = L.EncoderSaved(ops._p(fw["z_cat"]), ops._p(fw["z_fus"]), ops._p(gate), ops._p(fw["coef"][0]),
                        ops._p(fw["coef"][1]), ops._p(fw["coef"][2]), ops._p(fw["coef"][3]), ops._p(fw["argmax"]),
                        ops._p(fw["coef"][4]), int(recompute))
    g = [_nan(*t.shape) for t in p2]
    gr = L.EncoderGrads()
    for k in range(5):
        gr.conv[k] = L.BnLayerGrad(ops._p(g[2 * k]), ops._p(g[2 * k + 1]), ops._p(g[10 + 2 * k]), ops._p(g[11 + 2 * k]))
    gr.fusion = L.BnLayerGrad(ops._p(g[20]), ops._p(g[21]), ops._p(g[22]), ops._p(g[23]))
    gr.d_gate_w1, gr.d_gate_b1, gr.d_gate_w2, gr.d_gate_b2 = ops._p(g[24]), ops._p(g[25]), ops._p(g[26]), ops._p(g[27])
    dx = _nan(B, N, CIN)
    ws = ops._ws(d.device, lib.prh_encoder_workspace_bytes(B, N, CIN, OD, 2 if scratch else 1))
    rc = lib.prh_encoder_backward(C.byref(prm), ops._p(fw["x"]), B, N, 1, ops._p(d), ops._p(d_gfeat), int(scratch),
                                  C.byref(sv), C.byref(gr), ops._p(dx), ops._p(ws), ws.numel(), 0, ops._stream(d.device))
    torch.cuda.synchronize()
    return rc, dict(d_fused=d, dG=gate, dx=dx, grads=g)


@pytest.fixture(scope="module")
def forwards(lib, weights):
    """One storing and one gate-less forward per shape, shared by the tests below and left unchanged."""
    return {s: (_forward(lib, weights, *s, True), _forward(lib, weights, *s, False)) for s in SHAPES}


@pytest.mark.parametrize("B,N", SHAPES)
def test_forward_without_gate_buffer_is_the_same_forward(lib, forwards, B, N):
    assert lib.prh_encoder_gate_recompute(B, N, CIN, OD, 0) == 1
    a, b = forwards[(B, N)]
    Pn = B * N
    for k in ("fused", "z_fus", "z_cat", "coef"):
        assert _same(a[k], b[k]), k
    for u, v in zip(a["bufs"], b["bufs"]):
        assert torch.equal(u, v)
    assert not torch.isnan(a["fused"][:Pn]).any() and not torch.isnan(a["gate"][:Pn]).any()
    for k in ("fused", "z_fus", "z_cat", "gate"):          # rows beyond P untouched
        assert torch.isnan(a[k][Pn:]).all(), k
    assert float(a["gate"][:Pn].min()) >= 0.5 and float(a["gate"][:Pn].max()) <= 1.0


@pytest.mark.parametrize("B,N", SHAPES)
def test_step1_recompute_equals_stored_gate(lib, weights, forwards, B, N):
    fw = forwards[(B, N)][0]
    Pn, nb = B * N, (B * N + 63) // 64
    d0 = _d_fused(Pn, seed=N)
    rc0, dy0, dG0, a0, b0 = _step1(lib, weights, fw, B, N, 0, d0)
    rc1, dy1, dG1, a1, b1 = _step1(lib, weights, fw, B, N, 1, d0)
    assert rc0 == 0 and rc1 == 0, lib.prh_last_error()
    assert not torch.isnan(dy1[:Pn]).any() and not torch.isnan(dG1[:Pn]).any() and not torch.isnan(a1[:nb]).any()
    assert _same(dy0, dy1) and _same(dG0, dG1)
    assert _same(a0, a1) and _same(b0, b1)
    # rows beyond P and the sentinel row of the partials are untouched
    assert torch.isnan(dy1[Pn:]).all() and torch.isnan(dG1[Pn:]).all()
    assert torch.isnan(a1[nb:]).all() and torch.isnan(b1[nb:]).all()
    # the column sums of dy follow the contract's order, restated in numpy on the kernel's own dy
    ref = contract_partials(dy1[:Pn].cpu().numpy())
    assert np.array_equal(ref.view(np.int32), a1[:nb].cpu().numpy().view(np.int32))
    # the arithmetic of dy and dG, restated in torch on the stored gate (z*s+t exactly, through fp64)
    z, m, d = fw["z_fus"][:Pn], fw["gate"][:Pn], d0[:Pn]
    pre = (z.double() * fw["coef"][0, CAT:].double() + fw["coef"][1, CAT:].double()).float()
    sig = 2.0 * m - 1.0
    assert _same(torch.where(pre > 0, d * m, torch.zeros_like(d)), dy1[:Pn])
    assert _same(d * pre.clamp_min(0.0) * 0.5 * sig * (1.0 - sig), dG1[:Pn])


@pytest.mark.parametrize("B,N,scratch", [(8, 256, 1), (2, 1000, 1), (3, 683, 1), (2, 1000, 0)])
def test_backward_recompute_equals_stored_gate(lib, weights, forwards, B, N, scratch):
    fw_store, fw_none = forwards[(B, N)]
    Pn = B * N
    d0 = _d_fused(Pn, seed=7 + N)
    rc0, o0 = _backward(lib, weights, fw_store, B, N, 0, d0, scratch)
    rc1, o1 = _backward(lib, weights, fw_none, B, N, 1, d0, scratch)      # on the forward that stored no gate
    assert rc0 == 0 and rc1 == 0, lib.prh_last_error()
    assert _same(o0["dG"], o1["dG"]) and torch.isnan(o1["dG"][Pn:]).all() and not torch.isnan(o1["dG"][:Pn]).any()
    assert _same(o0["d_fused"], o1["d_fused"]) and torch.isnan(o1["d_fused"][Pn:]).all()
    if not scratch:
        assert _same(o1["d_fused"], d0)              # read only
    assert _same(o0["dx"], o1["dx"]) and not torch.isnan(o1["dx"]).any()
    from pointnet_refine_amd import ops
    for k, u, v in zip(ops.ENC_PARAM_ORDER, o0["grads"], o1["grads"]):
        assert _same(u, v), k
        assert not torch.isnan(v).any(), k


def test_below_the_grid_floor_the_stored_gate_path_stays(lib, weights):
    B, N = 2, 64
    Pn = B * N
    assert lib.prh_encoder_gate_recompute(B, N, CIN, OD, 0) == 0
    fw = _forward(lib, weights, B, N, True)
    d0 = _d_fused(Pn, seed=1)
    rc, dy, dG, a, b = _step1(lib, weights, fw, B, N, 0, d0)
    assert rc == 0, lib.prh_last_error()
    z, m, d = fw["z_fus"][:Pn], fw["gate"][:Pn], d0[:Pn]
    pre = (z.double() * fw["coef"][0, CAT:].double() + fw["coef"][1, CAT:].double()).float()
    sig = 2.0 * m - 1.0
    assert _same(torch.where(pre > 0, d * m, torch.zeros_like(d)), dy[:Pn])
    assert _same(d * pre.clamp_min(0.0) * 0.5 * sig * (1.0 - sig), dG[:Pn])
    assert np.array_equal(contract_partials(dy[:Pn].cpu().numpy()).view(np.int32), a[:2].cpu().numpy().view(np.int32))
    assert torch.isnan(dy[Pn:]).all() and torch.isnan(a[2:]).all()
    # asking for the recompute here is an error, not a fall-back
    assert _step1(lib, weights, fw, B, N, 1, d0)[0] != 0
    rc0, o0 = _backward(lib, weights, fw, B, N, 0, d0)
    assert rc0 == 0 and not any(torch.isnan(g).any() for g in o0["grads"])
    assert _backward(lib, weights, fw, B, N, 1, d0)[0] != 0


def test_pooled_output_takes_the_stored_gate_path(lib, weights):
    from pointnet_refine_amd import ops
    from pointnet_refine_amd.model import MultiScalePointNetEncoder
    B, N = 8, 256
    assert lib.prh_encoder_gate_recompute(B, N, CIN, OD, 1) == 0
    # C ABI: a pooled gradient with gate_recompute set is refused
    fw = _forward(lib, weights, B, N, True, want_global=True)
    dgf = torch.ones(B, 2 * OD, device="cuda")
    assert _backward(lib, weights, fw, B, N, 1, _d_fused(B * N, seed=2), scratch=0, d_gfeat=dgf)[0] != 0
    # module surface: with the pooled output the switch changes nothing
    sd = P.encoder_state_dict(CIN, OD, seed=3)
    x = P.synth_batch(B, N, CIN, 32, seed=11)[0].cuda()
    grads = []
    old = ops.GATE_RECOMPUTE
    try:
        for flag in (True, False):
            ops.GATE_RECOMPUTE = flag
            m = MultiScalePointNetEncoder(in_channel=CIN, out_dim=OD)
            m.load_state_dict(sd, strict=True)
            m = m.cuda().train()
            gf, fu = m(x.transpose(2, 1))
            (gf.sum() + (fu * fu).sum()).backward()
            grads.append([p.grad.clone() for p in m.parameters()])
    finally:
        ops.GATE_RECOMPUTE = old
    for u, v in zip(*grads):
        assert _same(u, v)


def test_training_step_gradients_do_not_depend_on_the_switch(lib):
    from pointnet_refine_amd import ops
    from pointnet_refine_amd.model import LineRefineNet
    B, N = 8, 256
    assert lib.prh_encoder_gate_recompute(B, N, CIN, OD, 0) == 1
    sd = P.linerefine_state_dict(0)
    ctx, noisy, target = P.synth_batch(B, N, CIN, 32, seed=7)
    res = []
    old = ops.GATE_RECOMPUTE
    try:
        for flag in (True, False):
            ops.GATE_RECOMPUTE = flag
            m = LineRefineNet()
            m.load_state_dict(sd, strict=True)
            m = m.cuda().train()
            for mod in m.modules():          # dropout off: both runs see the same network
                if isinstance(mod, torch.nn.Dropout):
                    mod.p = 0.0
                if isinstance(mod, torch.nn.MultiheadAttention):
                    mod.dropout = 0.0
            out = m(ctx.cuda(), noisy.cuda())
            loss = ops.deep_supervision_l1(out, target.cuda())
            loss.backward()
            torch.cuda.synchronize()
            res.append((loss.detach().clone(), {k: p.grad.clone() for k, p in m.named_parameters()}))
    finally:
        ops.GATE_RECOMPUTE = old
    assert _same(res[0][0], res[1][0])
    for k in res[0][1]:
        assert _same(res[0][1][k], res[1][1][k]), k
        assert not torch.isnan(res[0][1][k]).any(), k
