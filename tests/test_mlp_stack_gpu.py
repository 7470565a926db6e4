"""prh_mlp_stack_forward / prh_mlp_stack_backward at the C ABI against the fp64 reference of tests/_stack_ref.py.

The backward is compared on FORCED MASKS: every kernel decides a ReLU as fmaf(z, scale, shift) > 0 and the forward
returns z_cat, bn_scale and bn_shift, so the test recomputes each mask exactly (_stack_ref.device_masks) and runs the
reference backward on the device's saved forward with the device's masks.  What is left between the two is arithmetic
error, and the gates are the project's own for the same GEMM cores: forward max-abs 2e-5 * max(1, max|ref|), gradients
rel-L2 1e-5 per tensor, shared by modes 0, 1, 3 and 4.  The training-mode db is analytically zero and is measured
against sum|dz| of its columns.  The forward is compared with the reference on its own masks; device masks may differ
from those only where |y_ref| <= 2e-5 * max(1, max|y_ref|) of the layer.

Cases (tests/_stack_cases.py) are the smallest sizes that select each path of stack_forward / stack_backward;
test_the_cases_select_the_kernel_families_they_are_named_for restates the library's rules.  Every output starts from
NaN with guard rows in front and behind; running statistics and the counter are cloned per call; momentum = 0.25 and
eps = 3e-5 throughout.

Largest observed error / gate per quantity and mode over all cases but P = 2 (MI355X; every test prints its own):
    mode 0:  z 0.020  y 0.030  mean 0.017  rstd 0.007  scale 0.007  shift 0.009  running_mean 0.007  running_var 0.007
             dx 0.045  dw 0.054  dgamma 0.052  dbeta 0.050  db 0.001
    mode 1:  z 0.017  y 0.028  mean 0.015  rstd 0.007  scale 0.007  shift 0.009  running_mean 0.007  running_var 0.007
             dx 0.045  dw 0.056  dgamma 0.109  dbeta 0.144  db 0.001
    mode 3:  z 0.033  y 0.046  mean 0.021  rstd 0.008  scale 0.010  shift 0.009  running_mean 0.007  running_var 0.007
             dx 0.059  dw 0.088  dgamma 0.145  dbeta 0.246  db 0.067
    mode 4:  z 0.017  y 0.026  mean 0.015  rstd 0.007  scale 0.007  shift 0.009  running_mean 0.007  running_var 0.007
             dx 0.045  dw 0.070  dgamma 0.070  dbeta 0.088  db 0.001
Every mode keeps its claim of fp32-level accuracy with a factor of four or more to spare; no gate of the split cores
was widened.  Mask flips against the reference's own masks: 3 elements in all 27 cases together, every one inside the
band.  Band shares of the inputs (share of hidden post-BN values within the forward gate of zero, asserted <= 1e-3 by
tests/test_stack_ref_cpu.py): 0 to 2.0e-4, point_mlp at P = 8197 9.0e-5.

P = 2 (mode 3) is the one case with gates of its own, for dx, dw and db only (_stack_cases.TWO_ROW_GATES):
    z 0.020  y 0.246  mean 0.019  rstd 0.774  scale 0.774  shift 0.429  running_mean 0.007  running_var 0.013
    dgamma 0.714  dbeta 0.716   |   dx 213.7  dw 69.6  db 16.4  (x 1e-5; gates 800, 270, 64)
With two rows BatchNorm's backward cancels to eps / (var + eps) of its terms, 1e-6 and less with x in +-25, and the
kernels form dz = ca*dy + cb*z + cc from fp32 coefficient vectors: rounding those three vectors alone, all else in
fp64, gives 163.5 / 141.2 / 202.2 on the same inputs (tests/test_stack_ref_cpu.py).  That is the arithmetic of the
contract's form at this size, not a kernel's error; the gates are below four times the measured figures.

The gamma x 2^8 cases (_stack_cases.GAMMA_STACK) are there for one mistake: a split-fp16 operand scale read from the
neighbouring layer's header (stack_backward's `cur ^= 1`).  They make max|dz| of layer 2 1/1400 of layer 1's; a scale
placed for the smaller maximum leaves a factor 4 under fp16's largest number, so layer 1's dz overflows the planes and
its dw comes out NaN.  With the flip removed in a scratch build exactly that happens (both sizes; the 6-column and the
encoder-width stacks fail the same way), while the plain point_mlp cases at P >= 8192 stay inside the gates: their
adjacent maxima are 3 to 11 apart, which the headroom and 22 bits absorb.  The running maximum of the error ratios
keeps NaN (_worst): Python's max would drop it.

A defect the edge tests exposed and this change fixes: both entry points accepted a workspace up to 256 bytes shorter
than prh_mlp_stack_workspace_bytes reports (harmless by itself) and a NULL workspace with a non-zero size (not
harmless: every carved pointer is then NULL).  They now follow the rule of the bf16 Linear entry points.
"""
import ctypes as C

import numpy as np
import pytest
import torch

import _stack_cases as K
import _stack_ref as R

pytestmark = pytest.mark.gpu

GUARD = 4                         # sentinel rows in front of and behind every output (4 rows keep 16-byte alignment)
PRH_ERR_ARG, PRH_ERR_WORKSPACE = -1, -2


def test_the_cases_select_the_kernel_families_they_are_named_for():
    """csrc/prh_lib.hip's launch rules restated (tests/_stack_cases.py), so that a moved threshold does not silently
    turn these cases into repeats of one another.  fwd / dgrad / wgrad per layer; h2: second-generation split-fp16 NT
    core, h2tr: its transposed-read TN core, "+apply": held back to carry the apply pass of the layer below, s3:
    split-bf16 (first generation), direct / small: the one-launch TN kernels of prh_small.hpp."""
    f = {c.name: K.families(c) for c in K.CASES}
    pm = lambda P, m=3, t="train", rl=0: f[f"point_mlp_3x64x128x256_P{P}_m{m}_{t}_rl{rl}"]
    fp32 = dict(fwd=("fp32",) * 3, dgrad=("fp32",) * 3, wgrad=("fp32",) * 3)
    for P in (2, 77, 129, 513):                      # 513: M >= 512 but 3 row tiles of 256, below the 32-tile floor
        assert pm(P) == dict(fp32, mat=True)
    assert pm(77, 0) == dict(fp32, mat=False) and pm(77, 1) == dict(fp32, mat=False) and pm(77, 4) == dict(fp32, mat=True)
    assert pm(8000) == dict(fwd=("fp32", "h2", "h2"), dgrad=("fp32", "fp32", "h2"), wgrad=("fp32",) * 3, mat=True)
    held = dict(fwd=("fp32", "h2", "h2"), dgrad=("fp32", "fp32", "h2"), wgrad=("fp32", "h2tr+apply", "h2tr+apply"), mat=True)
    assert pm(8192) == held and pm(8197) == held and pm(8197, 4) == held
    assert pm(8197, rl=1) == held and pm(8197, t="eval") == held and pm(8197, t="eval", rl=1) == held
    assert pm(8192, 0) == dict(fp32, mat=False) and pm(8197, 0) == dict(fp32, mat=False)
    assert pm(8197, 1) == dict(fwd=("fp32", "s3", "s3"), dgrad=("fp32", "fp32", "s3"), wgrad=("fp32", "s3", "s3"), mat=False)
    for P in (8192, 8197):
        assert f[f"gamma256_3x64x128x512_P{P}_m3_train_rl0"] == dict(
            fwd=("fp32", "h2", "h2"), dgrad=("fp32", "fp32", "h2"), wgrad=("fp32", "h2tr+apply", "h2tr+apply"), mat=True)
    assert f["seeded_6x64x128x256x512_P8197_m3_train_rl0"] == dict(
        fwd=("fp32", "h2", "h2", "h2"), dgrad=("fp32", "fp32", "h2", "h2"),
        wgrad=("fp32", "h2tr+apply", "h2tr+apply", "h2tr+apply"), mat=True)
    assert f["seeded_4x64x128x256x512x1024_P8197_m3_train_rl0"] == dict(
        fwd=("fp32", "h2", "h2", "h2", "h2"), dgrad=("fp32", "fp32", "h2", "h2", "h2"),
        wgrad=("fp32",) + ("h2tr+apply",) * 4, mat=True)
    small = lambda P: f[f"seeded_64x128x64_P{P}_m3_train_rl0"]["wgrad"]
    assert small(256) == ("direct", "fp32") and small(4160) == ("small", "fp32") and small(250) == ("fp32", "fp32")
    assert all(v["fwd"] == v["dgrad"] == ("fp32", "fp32") for k, v in f.items() if k.startswith("seeded_64x128x64"))


# ------------------------------------------------------------------------------------------ plumbing
def _p(t):
    return C.c_void_p(0 if t is None or t.numel() == 0 else t.data_ptr())


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _guarded(rows, width):
    """A (rows, width) NaN view with GUARD NaN rows on either side; returns (view, whole)."""
    whole = torch.full((rows + 2 * GUARD, width), float("nan"), dtype=torch.float32, device="cuda")
    return whole[GUARD:GUARD + rows], whole


def _guards_intact(whole):
    return bool(torch.isnan(whole[:GUARD]).all() and torch.isnan(whole[-GUARD:]).all())


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


class Stack:
    """Device copies of an input set and the two entry points around them."""

    def __init__(self, lib, key):
        self.lib, self.key = lib, key
        self.widths, self.P, self.training, self.relu_last, _ = key
        layers, running, x, dy = K.inputs(key)
        self.nl = len(layers)
        self.cout = list(self.widths[1:])
        self.ctot = sum(self.cout)
        self.off = [0] + list(np.cumsum(self.cout))
        dev = lambda a: torch.from_numpy(np.array(a)).cuda()
        self.params = [{k: dev(v) for k, v in ly.items()} for ly in layers]
        self.running0 = [(dev(rm), dev(rv)) for rm, rv in running]
        self.nbt0 = [torch.tensor(11 + l, dtype=torch.int64, device="cuda") for l in range(self.nl)]
        self.x, self.dy = dev(x), dev(dy)

    def structs(self, bufs, with_nbt=True):
        from pointnet_refine_amd import _lib as L
        arr = (L.BnLayer * self.nl)()
        for l, p in enumerate(self.params):
            rm, rv, nbt = bufs[l]
            arr[l] = L.BnLayer(_p(p["w"]), _p(p["b"]), _p(p["gamma"]), _p(p["beta"]), _p(rm), _p(rv),
                               _p(nbt if with_nbt else None), p["w"].shape[1], p["w"].shape[0])
        return arr

    def workspace_bytes(self, P=None):
        bufs = [(rm, rv, n) for (rm, rv), n in zip(self.running0, self.nbt0)]
        return int(self.lib.prh_mlp_stack_workspace_bytes(self.P if P is None else P, self.nl, self.structs(bufs)))

    def forward(self, with_nbt=True, ws=None, ws_bytes=None, P=None, training=None):
        P = self.P if P is None else P
        training = self.training if training is None else training
        bufs = [(rm.clone(), rv.clone(), n.clone()) for (rm, rv), n in zip(self.running0, self.nbt0)]
        z_cat, z_whole = _guarded(P, self.ctot)
        y, y_whole = _guarded(P, self.cout[-1])
        coef = [_vec(self.ctot) for _ in range(4)]          # scale, shift, mean, rstd
        if ws is None:
            ws = torch.empty(self.workspace_bytes(P), dtype=torch.uint8, device="cuda")
        nbytes = ws.numel() if ws_bytes is None else ws_bytes
        rc = self.lib.prh_mlp_stack_forward(self.structs(bufs, with_nbt), self.nl, self.relu_last, _p(self.x), P,
                                            training, K.MOMENTUM, K.EPS, _p(z_cat), _p(y), _p(coef[0][0]),
                                            _p(coef[1][0]), _p(coef[2][0]), _p(coef[3][0]), _p(ws), nbytes, 0, _stream())
        torch.cuda.synchronize()
        return rc, dict(z_cat=z_cat, y=y, scale=coef[0][0], shift=coef[1][0], mean=coef[2][0], rstd=coef[3][0],
                        wholes=[z_whole, y_whole] + [c[1] for c in coef], bufs=bufs, P=P, training=training)

    def backward(self, fw, want_dx=True, want_grads=True, skip_dw=(), ws=None, ws_bytes=None):
        from pointnet_refine_amd import _lib as L
        P = fw["P"]
        grads, wholes = [], []
        arr = (L.BnLayerGrad * self.nl)()
        for l, p in enumerate(self.params):
            dw, dw_whole = _guarded(*p["w"].shape)
            vecs = [_vec(self.cout[l]) for _ in range(3)]
            g = dict(dw=None if l in skip_dw else dw, db=vecs[0][0], dgamma=vecs[1][0], dbeta=vecs[2][0])
            arr[l] = L.BnLayerGrad(_p(g["dw"]), _p(g["db"]), _p(g["dgamma"]), _p(g["dbeta"]))
            grads.append(g)
            wholes += [dw_whole] + [v[1] for v in vecs]
        dx, dx_whole = _guarded(P, self.widths[0])
        wholes.append(dx_whole)
        # the backward reads gamma alone of the parameters besides w; statistics are not touched (NULL counter)
        bufs = [(rm, rv, None) for rm, rv in self.running0]
        if ws is None:
            ws = torch.empty(self.workspace_bytes(P), dtype=torch.uint8, device="cuda")
        nbytes = ws.numel() if ws_bytes is None else ws_bytes
        rc = self.lib.prh_mlp_stack_backward(self.structs(bufs, False), self.nl, self.relu_last, _p(self.x), P,
                                             fw["training"], _p(self.dy), _p(fw["z_cat"]), _p(fw["scale"]),
                                             _p(fw["shift"]), _p(fw["mean"]), _p(fw["rstd"]),
                                             arr if want_grads else None, _p(dx if want_dx else None), _p(ws), nbytes,
                                             0, _stream())
        torch.cuda.synchronize()
        return rc, dict(dx=dx, grads=grads, wholes=wholes)


def _check_forward(st, fw, ref, with_nbt=True):
    """Error / gate of every forward quantity (<= 1 passes), the device masks, and the list of hard failures."""
    nl, off, bad = st.nl, st.off, []
    if not all(_guards_intact(w) for w in fw["wholes"]):
        bad.append("forward wrote into a guard row")
    z_cat = _np(fw["z_cat"])
    co = {k: _np(fw[k]) for k in ("scale", "shift", "mean", "rstd")}
    q = dict(z=0.0, y=0.0, mean=0.0, rstd=0.0, scale=0.0, shift=0.0, running_mean=0.0, running_var=0.0)
    masks = R.device_masks(z_cat, co["scale"], co["shift"], st.cout)
    flips = 0
    for l in range(nl):
        s = slice(off[l], off[l + 1])
        q["z"] = _worst(q["z"], K.fwd_ratio(ref[l]["z"], z_cat[:, s]))
        for k in ("mean", "rstd", "scale", "shift"):
            q[k] = _worst(q[k], K.fwd_ratio(ref[l][k], co[k][s]))
        rm, rv, nbt = fw["bufs"][l]
        if fw["training"]:
            q["running_mean"] = _worst(q["running_mean"], K.fwd_ratio(ref[l]["running_mean"], _np(rm)))
            q["running_var"] = _worst(q["running_var"], K.fwd_ratio(ref[l]["running_var"], _np(rv)))
        elif not (_same(rm, st.running0[l][0]) and _same(rv, st.running0[l][1])):
            bad.append(f"eval mode touched the running statistics of layer {l}")
        want = int(st.nbt0[l]) + (1 if fw["training"] and with_nbt else 0)
        if int(nbt) != want:
            bad.append(f"num_batches_tracked of layer {l}: {int(nbt)}, expected {want}")
        # the post-BN value every consumer rebuilds from the saved z, scale and shift
        y_dev = z_cat[:, s].astype(np.float64) * co["scale"][s].astype(np.float64) + co["shift"][s].astype(np.float64)
        q["y"] = _worst(q["y"], K.fwd_ratio(ref[l]["y"], y_dev))
        if R.has_relu(l, nl, st.relu_last):
            flip = masks[l] != ref[l]["mask"]
            flips += int(flip.sum())
            if (flip & (np.abs(ref[l]["y"]) > R.band(ref[l]["y"], K.GATE_FWD, 1.0))).any():
                bad.append(f"layer {l}: a ReLU mask differs from the reference's outside the band")
    q["y"] = _worst(q["y"], K.fwd_ratio(ref[-1]["out"], _np(fw["y"])))
    return q, masks, flips, bad


def _reference_backward(st, fw, masks):
    layers, _, x, dy = K.inputs(st.key)
    recs = R.records_from_saved(_np(fw["z_cat"]), _np(fw["scale"]), _np(fw["shift"]), _np(fw["mean"]),
                                _np(fw["rstd"]), st.cout, st.relu_last, masks)
    return R.backward(dy, x, layers, recs, fw["training"], st.relu_last, masks)


def _check_backward(st, fw, bw, dx_ref, g_ref, skip_dw=()):
    q, bad = dict(dx=K.grad_ratio(dx_ref, _np(bw["dx"])), dw=0.0, dgamma=0.0, dbeta=0.0, db=0.0), []
    if not all(_guards_intact(w) for w in bw["wholes"]):
        bad.append("backward wrote into a guard row")
    for l in range(st.nl):
        g = bw["grads"][l]
        for k in ("dw", "dgamma", "dbeta"):
            if k == "dw" and l in skip_dw:
                continue
            q[k] = _worst(q[k], K.grad_ratio(g_ref[l][k], _np(g[k])))
        if fw["training"]:
            q["db"] = _worst(q["db"], K.db_ratio(g_ref[l]["db"], _np(g["db"]), g_ref[l]["dz"]))
        else:
            q["db"] = _worst(q["db"], K.grad_ratio(g_ref[l]["db"], _np(g["db"])))
            if not np.abs(_np(g["db"])).max() > 0:
                bad.append(f"eval-mode db of layer {l} is zero")
    return q, bad


def _verdict(tag, q, bad, limits={}):
    print(tag, " ".join(f"{k}={v:.3f}" for k, v in q.items()), "|", "; ".join(bad) if bad else "ok")
    over = {k: round(v, 3) for k, v in q.items() if not v <= limits.get(k, 1.0)}
    assert not bad and not over, (tag, bad, over)


# ------------------------------------------------------------------------------------------ the cases
@pytest.mark.parametrize("case", K.CASES, ids=[c.name for c in K.CASES])
def test_stack_forward_and_backward_against_fp64(lib_mode, case):
    lib = lib_mode(case.mode)
    st = Stack(lib, case.inputs)
    ref = K.reference_forward(case.inputs)
    rc, fw = st.forward()
    assert rc == 0, lib.prh_last_error()
    qf, masks, flips, bad = _check_forward(st, fw, ref)
    dx_ref, g_ref = _reference_backward(st, fw, masks)
    rc, bw = st.backward(fw)
    assert rc == 0, lib.prh_last_error()
    qb, bad_b = _check_backward(st, fw, bw, dx_ref, g_ref)
    _verdict(f"STACK {case.name} mode={case.mode} flips={flips}", {**qf, **qb}, bad + bad_b, K.limits(case.P))


# ------------------------------------------------------------------------------------------ contract edges
SMALL = K.Case(K.POINT_MLP, 77, weights="point_mlp")
BIG = K.Case(K.POINT_MLP, 8197, weights="point_mlp")      # both held wgrads carry an apply pass


@pytest.fixture(scope="module")
def big():
    """One forward, its masks, the reference backward and one full backward of the P = 8197 point_mlp case in mode 3,
    shared by the edge tests below and left unchanged."""
    from pointnet_refine_amd import _lib
    lib = _lib.lib()
    old = lib.prh_get_gemm_mode()
    lib.prh_set_gemm_mode(3)
    try:
        st = Stack(lib, BIG.inputs)
        rc, fw = st.forward()
        assert rc == 0, lib.prh_last_error()
        masks = R.device_masks(_np(fw["z_cat"]), _np(fw["scale"]), _np(fw["shift"]), st.cout)
        dx_ref, g_ref = _reference_backward(st, fw, masks)
        rc, bw = st.backward(fw)
        assert rc == 0, lib.prh_last_error()
    finally:
        lib.prh_set_gemm_mode(old)
    return dict(st=st, fw=fw, bw=bw, dx_ref=dx_ref, g_ref=g_ref)


def _grads_same(a, b, skip_dw=()):
    return all(_same(ga[k], gb[k]) for l, (ga, gb) in enumerate(zip(a["grads"], b["grads"])) for k in ga
               if not (k == "dw" and l in skip_dw))


def test_training_needs_two_rows_and_eval_does_not(lib_mode):
    lib = lib_mode(3)
    st = Stack(lib, K.Case(K.POINT_MLP, 77, training=0, weights="point_mlp").inputs)
    rc, _ = st.forward(P=1, training=1)
    assert rc == PRH_ERR_ARG and b"more than 1 value" in lib.prh_last_error()
    rc, fw = st.forward(P=1, training=0)
    assert rc == 0, lib.prh_last_error()
    layers, running, x, _ = K.inputs(st.key)
    ref = R.forward(x[:1], layers, 0, K.MOMENTUM, K.EPS, 0, running)
    assert K.fwd_ratio(ref[-1]["out"], _np(fw["y"])) <= 1.0 and all(_guards_intact(w) for w in fw["wholes"])


def test_bad_layer_chains_are_refused(lib_mode):
    lib = lib_mode(3)
    st = Stack(lib, SMALL.inputs)
    bufs = [(rm.clone(), rv.clone(), n.clone()) for (rm, rv), n in zip(st.running0, st.nbt0)]
    z, y, v = torch.zeros(77, 448, device="cuda"), torch.zeros(77, 256, device="cuda"), torch.zeros(4, 448, device="cuda")
    ws = torch.empty(st.workspace_bytes(), dtype=torch.uint8, device="cuda")
    for bad_widths, cins, text in (((64, 126, 256), (3, 64, 126), b"multiple of 4"),
                                   ((64, 128, 256), (3, 60, 128), b"previous cout")):
        arr = st.structs(bufs)
        for l in range(3):
            arr[l].cin, arr[l].cout = cins[l], bad_widths[l]
        rc = lib.prh_mlp_stack_forward(arr, 3, 0, _p(st.x), 77, 1, K.MOMENTUM, K.EPS, _p(z), _p(y), _p(v[0]), _p(v[1]),
                                       _p(v[2]), _p(v[3]), _p(ws), ws.numel(), 0, _stream())
        assert rc == PRH_ERR_ARG and text in lib.prh_last_error(), lib.prh_last_error()
        rc = lib.prh_mlp_stack_backward(arr, 3, 0, _p(st.x), 77, 1, _p(st.dy), _p(z), _p(v[0]), _p(v[1]), _p(v[2]),
                                        _p(v[3]), None, None, _p(ws), ws.numel(), 0, _stream())
        assert rc == PRH_ERR_ARG and text in lib.prh_last_error(), lib.prh_last_error()
    torch.cuda.synchronize()
    for (rm, rv, n), (rm0, rv0), n0 in zip(bufs, st.running0, st.nbt0):      # a refused call changes nothing
        assert _same(rm, rm0) and _same(rv, rv0) and int(n) == int(n0)


@pytest.mark.parametrize("mode", [0, 3])
def test_a_workspace_one_byte_short_is_refused(lib_mode, mode):
    lib = lib_mode(mode)
    st = Stack(lib, SMALL.inputs)
    n = st.workspace_bytes()
    ws = torch.empty(n, dtype=torch.uint8, device="cuda")
    rc, fw = st.forward(ws=ws, ws_bytes=n - 1)
    assert rc == PRH_ERR_WORKSPACE, lib.prh_last_error()
    assert torch.isnan(fw["y"]).all() and all(int(b[2]) == int(n0) for b, n0 in zip(fw["bufs"], st.nbt0))
    rc, fw = st.forward(ws=ws)
    assert rc == 0
    rc, bw = st.backward(fw, ws=ws, ws_bytes=n - 1)
    assert rc == PRH_ERR_WORKSPACE, lib.prh_last_error()
    assert torch.isnan(bw["dx"]).all()
    # (reached only past the refusals above) a missing workspace is refused the same way, whatever size is claimed
    rc, fw2 = st.forward(ws=torch.empty(0, dtype=torch.uint8, device="cuda"), ws_bytes=n)
    assert rc == PRH_ERR_WORKSPACE and torch.isnan(fw2["y"]).all(), lib.prh_last_error()
    rc, bw = st.backward(fw, ws=torch.empty(0, dtype=torch.uint8, device="cuda"), ws_bytes=n)
    assert rc == PRH_ERR_WORKSPACE and torch.isnan(bw["dx"]).all(), lib.prh_last_error()


@pytest.mark.parametrize("case", [SMALL, BIG, K.Case(K.POINT_MLP, 8197, mode=1, weights="point_mlp"),
                                  K.Case((6, 64, 128, 256, 512), 8197)], ids=lambda c: c.name)
def test_the_reported_workspace_size_is_enough(lib_mode, case):
    """Inside a larger allocation whose tail beyond the reported size holds a byte pattern, and whose head starts from
    NaN bits instead of whatever the allocator left: the pattern survives and every output has the bits of the normal
    run."""
    lib = lib_mode(case.mode)
    st = Stack(lib, case.inputs)
    n, tail = st.workspace_bytes(), 1 << 16
    rc, fw0 = st.forward()
    assert rc == 0, lib.prh_last_error()
    rc, bw0 = st.backward(fw0)
    assert rc == 0, lib.prh_last_error()

    def fresh():
        ws = torch.empty(n + tail, dtype=torch.uint8, device="cuda")
        ws[:n] = 0xFF
        ws[n:] = 0xA5
        return ws
    ws = fresh()
    rc, fw1 = st.forward(ws=ws, ws_bytes=n)
    assert rc == 0, lib.prh_last_error()
    assert bool((ws[n:] == 0xA5).all())
    ws = fresh()
    rc, bw1 = st.backward(fw1, ws=ws, ws_bytes=n)
    assert rc == 0, lib.prh_last_error()
    assert bool((ws[n:] == 0xA5).all())
    for k in ("z_cat", "y", "scale", "shift", "mean", "rstd"):
        assert _same(fw0[k], fw1[k]), k
    for b0, b1 in zip(fw0["bufs"], fw1["bufs"]):
        assert _same(b0[0], b1[0]) and _same(b0[1], b1[1]) and int(b0[2]) == int(b1[2])
    assert _same(bw0["dx"], bw1["dx"]) and _grads_same(bw0, bw1)
    assert not any(torch.isnan(g[k]).any() for g in bw1["grads"] for k in g) and not torch.isnan(bw1["dx"]).any()


def test_num_batches_tracked_may_be_null(lib_mode):
    lib = lib_mode(3)
    st = Stack(lib, SMALL.inputs)
    rc, fw = st.forward(with_nbt=False)
    assert rc == 0, lib.prh_last_error()
    q, _, _, bad = _check_forward(st, fw, K.reference_forward(SMALL.inputs), with_nbt=False)
    _verdict("STACK nbt=NULL", q, bad)


def test_null_dx_and_null_grads_leave_the_rest_bit_equal(lib_mode, big):
    st, fw, bw = big["st"], big["fw"], big["bw"]
    lib_mode(3)
    rc, no_dx = st.backward(fw, want_dx=False)
    assert rc == 0, st.lib.prh_last_error()
    assert _grads_same(bw, no_dx) and torch.isnan(no_dx["dx"]).all() and all(_guards_intact(w) for w in no_dx["wholes"])
    rc, no_g = st.backward(fw, want_grads=False)
    assert rc == 0, st.lib.prh_last_error()
    assert _same(bw["dx"], no_g["dx"]) and all(_guards_intact(w) for w in no_g["wholes"])
    assert all(torch.isnan(g[k]).all() for g in no_g["grads"] for k in g)


def test_a_null_dw_in_the_middle_breaks_the_held_chain_cleanly(lib_mode, big):
    """Without layer 1's dw there is no wgrad to hold: layer 0's apply pass runs on its own and measures its own
    maximum.  Everything else stays within the gates of the full run."""
    st, fw = big["st"], big["fw"]
    lib_mode(3)
    rc, bw = st.backward(fw, skip_dw=(1,))
    assert rc == 0, st.lib.prh_last_error()
    q, bad = _check_backward(st, fw, bw, big["dx_ref"], big["g_ref"], skip_dw=(1,))
    _verdict("STACK dw1=NULL", q, bad)


def test_two_backward_calls_from_one_forward_are_bit_equal(lib_mode, big):
    st, fw, bw = big["st"], big["fw"], big["bw"]
    lib_mode(3)
    keep = {k: fw[k].clone() for k in ("z_cat", "scale", "shift", "mean", "rstd")}
    rc, again = st.backward(fw)
    assert rc == 0, st.lib.prh_last_error()
    assert _same(bw["dx"], again["dx"]) and _grads_same(bw, again)
    assert all(_same(keep[k], fw[k]) for k in keep)          # nothing the backward needs is consumed
