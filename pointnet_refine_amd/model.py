"""Drop-in nn.Module surface of the reference's ``src/model.py`` on the MI355X HIP path.

Same class names, constructor signatures, ``forward`` contracts and ``state_dict`` (205
entries, names/shapes/dtypes of ``/root/reference/src/model.py``), so the reference's
``train.py`` / ``train_dist.py`` / ``inference_whole_scene.py`` work after replacing
``from src.model import LineRefineNet`` with ``from pointnet_refine_amd.model import
LineRefineNet`` and a strict ``load_state_dict`` of a reference checkpoint succeeds.

The submodules (``nn.Conv1d``, ``nn.BatchNorm1d``, ``nn.Linear`` ...) exist as PARAMETER
CONTAINERS with the reference's names and default initialisation; the arithmetic of every
row of SURVEY.md section 8a does not go through them but through ``ops.py`` -> C ABI ->
hand-written gfx950 kernels:

  a1-a4  MultiScalePointNetEncoder   ops.encoder / ops.encoder_eval_fused   (src/model.py:39-62)
  a5     context_proj                ops.linear                             (src/model.py:147,194)
  a6     point_mlp                   ops.mlp_stack                          (src/model.py:150-159,200-201)
  a7     regression heads            ops.linear (ReLU epilogue) + ops.linear_small   (:172-179,220)
  a9     PositionalEncoding          ops.pos_hidden + ops.linear (residual epilogue) (:64-75)
  a10    DETR decoder layers         ops.linear, ops.attention / attention_block,
                                     ops.add_dropout_layernorm                       (:77-135)

What is left to PyTorch is plumbing: the autograd graph and ``torch.stack``.  There is NO
stock-PyTorch arithmetic branch: shapes the kernels do not take (widths that are not multiples of 4,
heads that are not 32 wide, a d_model other than 256 in the LayerNorm pass) raise ``RuntimeError`` from
``ops.py`` / the C ABI, like CPU tensors do.
"""
from __future__ import annotations

import torch
import torch.nn as nn
import torch.nn.functional as F

from . import ops


def _warn_saturated(e):
    import warnings
    warnings.warn(f"{e} - falling back to the per-layer HIP kernels for this call", RuntimeWarning, stacklevel=3)


def _bn_buffers(bn: nn.BatchNorm1d):
    return [bn.running_mean, bn.running_var, bn.num_batches_tracked]


def _attn(q, k, v, heads, dropout_p):
    """softmax(q k^T / sqrt(d)) v with dropout on the attention weights: the fused HIP kernel pair
    (heads of 32 channels; anything else raises in ops.attention)."""
    seed = int(torch.randint(0, 2 ** 31 - 1, (1,)).item()) if dropout_p > 0.0 else 0
    return ops.attention(q, k, v, heads, dropout_p, seed)


def _add_norm(x, r, norm, drop, training):
    """norm(x + dropout(r)): one HIP pass each way (row f1; 256 channels, affine LayerNorm)."""
    if not norm.elementwise_affine:
        raise RuntimeError("pointnet_refine_amd: LayerNorm without affine parameters is not supported by the HIP path")
    return ops.add_dropout_layernorm(x, r, norm, drop.p if training else 0.0)


def _lin(x, weight, bias):
    """nn.Linear arithmetic on the HIP GEMM cores (in / out features multiples of 4; ops.linear raises
    otherwise - the 3-wide layers of the model have their own one-pass kernels)."""
    return ops.linear(x, weight, bias)


class MultiScalePointNetEncoder(nn.Module):
    """Multi-scale PointNet encoder with dual pooling (reference: src/model.py:5-62)."""

    GATE_HIDDEN = 64

    def __init__(self, in_channel=4, out_dim=1024):
        super().__init__()
        # Parameter containers only (names, shapes, default initialisers and registration
        # order of the reference's state_dict); the kernels read their tensors directly.
        widths = (in_channel, 64, 128, 256, 512, out_dim)
        for k in range(1, 6):
            self.add_module(f"conv{k}", nn.Conv1d(widths[k - 1], widths[k], kernel_size=1))
        for k in range(1, 6):
            self.add_module(f"bn{k}", nn.BatchNorm1d(widths[k]))
        self.fusion = nn.Sequential(nn.Conv1d(sum(widths[1:]), out_dim, kernel_size=1),
                                    nn.BatchNorm1d(out_dim), nn.ReLU())
        self.intensity_gate = nn.Sequential(nn.Conv1d(1, self.GATE_HIDDEN, kernel_size=1), nn.ReLU(),
                                            nn.Conv1d(self.GATE_HIDDEN, out_dim, kernel_size=1),
                                            nn.Sigmoid())
        self.in_channel, self.out_dim = in_channel, out_dim
        # inference (eval mode under torch.no_grad()): "fp32" / "fp16" = the single fused kernel with
        # BatchNorm folded (two fp16 planes, fp32-level error / one fp16 plane, BASELINE config 5);
        # None = the per-layer kernels that also serve training
        self.inference_precision = "fp32"

    def _fused_ok(self, x):
        return (self.inference_precision in ("fp32", "fp16") and not self.training and not torch.is_grad_enabled()
                and x.is_cuda and x.dtype == torch.float32 and self.out_dim == 1024
                and ops.encoder_eval_fused_supported(self._param_list()))

    def _param_list(self):
        sd = dict(self.named_parameters())
        return [sd[k] for k in ops.ENC_PARAM_ORDER]

    def _bn_buffer_list(self):
        b = []
        for bn in (self.bn1, self.bn2, self.bn3, self.bn4, self.bn5, self.fusion[1]):
            b += _bn_buffers(bn)
        return b

    def forward_pointmajor(self, x_pm: torch.Tensor, want_global: bool = True):
        """x_pm (B,N,C) contiguous point-major -> (global_feat (B,2*out) or None,
        fused (B,N,out)).  The layout the kernels use; LineRefineNet calls this directly
        and skips the pooling it would discard (src/model.py:193)."""
        if x_pm.dim() != 3:
            raise RuntimeError(f"Expected 3D (batched) input, but got input of size: {list(x_pm.shape)}")
        bn = self.bn1
        if self._fused_ok(x_pm):
            try:
                _, fused, gfeat = ops.encoder_eval_fused(x_pm, self._param_list(), self._bn_buffer_list(), bn.eps,
                                                         want_fused=True, want_global=want_global,
                                                         precision=self.inference_precision)
                return gfeat, fused
            except ops.FusedSaturation as e:      # activations beyond the fp16 range: the per-layer kernels take it
                _warn_saturated(e)
        return ops.encoder(x_pm, self._param_list(), self._bn_buffer_list(), want_global, self.training,
                           bn.momentum, bn.eps)

    def forward(self, x):
        """x: (B, C, N), C = 4 -> [x, y, z, intensity].  Returns (global_feat (B, 2*out_dim),
        fused (B, out_dim, N)) exactly like the reference (src/model.py:39-62)."""
        if x.dim() != 3:
            raise RuntimeError(f"Expected 3D (batched) input, but got input of size: {list(x.shape)}")
        gfeat, fused = self.forward_pointmajor(x.transpose(2, 1).contiguous(), True)
        if fused.dtype != x.dtype:              # bf16 mode keeps `fused` in bf16; the API contract is the input's dtype
            fused = fused.to(x.dtype)
        return gfeat, fused.transpose(2, 1)


class PositionalEncoding(nn.Module):
    """MLP positional encoding for 3-D coordinates (reference: src/model.py:64-75)."""

    def __init__(self, in_dim=3, out_dim=256):
        super().__init__()
        self.mlp = nn.Sequential(nn.Linear(in_dim, out_dim), nn.ReLU(), nn.Linear(out_dim, out_dim))

    def hidden(self, xyz):
        """(h, max h): Linear(3,H)+ReLU as one elementwise HIP pass over the points in place (a 3-deep GEMM is
        HBM work); the pass also reports h's largest value (None where nothing consumes it, ops.PRODUCER_MAXIMA)."""
        l0, l2 = self.mlp[0], self.mlp[2]
        if l0.in_features != 3 or not ops.pos_hidden_supported(l0.out_features) or l2.out_features % 4:
            raise RuntimeError(f"pointnet_refine_amd: PositionalEncoding({l0.in_features}, {l2.out_features}) is not "
                               "supported by the HIP path (3-wide points, power-of-two hidden width <= 1024)")
        return ops.pos_hidden_with_amax(xyz, l0.weight, l0.bias)

    def forward(self, xyz, resid=None):
        """resid: optional tensor added to the encoding (the decoder's k-input memory + pos,
        src/model.py:123-126) - on the GPU it rides on the second Linear's epilogue."""
        l2 = self.mlp[2]
        h, h_amax = self.hidden(xyz)
        # Linear(H,H) (+ resid) on the HIP GEMM cores.  With a residual (the context side: B*N rows) h's maximum
        # feeds the GEMM and the output's maximum is noted on the result for the Linear that reads it next
        if resid is None:
            return ops.linear(h, l2.weight, l2.bias, h_amax)
        y, y_amax = ops.linear_with_amax(h, l2.weight, l2.bias, h_amax, False, resid)
        ops.amax_note(y, y_amax)
        return y


class DetrTransformerDecoderLayer(nn.Module):
    """Post-norm DETR decoder layer (reference: src/model.py:77-135)."""

    def __init__(self, d_model=256, nhead=8, dim_feedforward=1024, dropout=0.1):
        super().__init__()
        # containers in the reference's registration order (state_dict keys self_attn.*,
        # cross_attn.*, linear1/2.*, norm1..3.*); nn.MultiheadAttention only stores the packed
        # in_proj / out_proj parameters here, its forward is never called
        for name in ("self_attn", "cross_attn"):
            self.add_module(name, nn.MultiheadAttention(d_model, nhead, dropout=dropout, batch_first=True))
        self.linear1 = nn.Linear(d_model, dim_feedforward)
        self.dropout = nn.Dropout(dropout)
        self.linear2 = nn.Linear(dim_feedforward, d_model)
        for k in (1, 2, 3):
            self.add_module(f"norm{k}", nn.LayerNorm(d_model))
        for k in (1, 2, 3):
            self.add_module(f"dropout{k}", nn.Dropout(dropout))
        self.activation = F.relu

    def with_pos_embed(self, tensor, pos):
        return tensor if pos is None else tensor + pos

    def forward(self, tgt, memory, query_pos=None, pos=None):
        """The reference's call contract (src/model.py:103-135): projects this layer's keys
        (memory + pos) and values (memory) on the HIP GEMM cores and runs the shared body."""
        ca, d = self.cross_attn, self.cross_attn.embed_dim
        k_proj = _lin(self.with_pos_embed(memory, pos), ca.in_proj_weight[d:2 * d], ca.in_proj_bias[d:2 * d])
        v_proj = _lin(memory, ca.in_proj_weight[2 * d:], ca.in_proj_bias[2 * d:])
        return self.forward_projected(tgt, k_proj, v_proj, query_pos=query_pos)

    def forward_projected(self, tgt, k_proj, v_proj, query_pos=None, kv_block=None):
        """Same layer with the cross-attention key/value projections already applied
        (k_proj = (memory+pos) Wk^T + bk, v_proj = memory Wv^T + bv, each (B,N,C), possibly a
        strided column block).  nn.MultiheadAttention's semantics written out: 8 heads of 32
        contiguous channels, scale 1/sqrt(32), dropout on the attention weights."""
        sa = self.self_attn
        d, h = sa.embed_dim, sa.num_heads
        B, M, _ = tgt.shape
        qk_in = self.with_pos_embed(tgt, query_pos)
        qk = _lin(qk_in, sa.in_proj_weight[:2 * d], sa.in_proj_bias[:2 * d])      # q and k share the input
        vv = _lin(tgt, sa.in_proj_weight[2 * d:], sa.in_proj_bias[2 * d:])
        pdrop_sa = sa.dropout if self.training else 0.0
        seed_sa = int(torch.randint(0, 2 ** 31 - 1, (1,)).item()) if pdrop_sa > 0.0 else 0
        o = ops.attention_self_packed(qk, vv, h, pdrop_sa, seed_sa)      # q / k read in place, dq / dk in one buffer
        tgt2 = _lin(o, sa.out_proj.weight, sa.out_proj.bias)
        tgt = _add_norm(tgt, tgt2, self.norm1, self.dropout1, self.training)
        ca = self.cross_attn
        qp = _lin(self.with_pos_embed(tgt, query_pos), ca.in_proj_weight[:d], ca.in_proj_bias[:d])
        pdrop = ca.dropout if self.training else 0.0
        if kv_block is not None and kv_block[0] == "fold":
            # inference: attention over the raw memory rows, this layer's key / value projections
            # folded into the kernel (k_proj / v_proj are the bf16 row images of memory + pos / memory)
            o = ops.attention_folded(qp, k_proj, v_proj, ca.in_proj_weight[d:2 * d], ca.in_proj_weight[2 * d:],
                                     ca.in_proj_bias[2 * d:], h)
        elif kv_block is not None:      # k_proj / v_proj are the wide buffers, kv_block picks the block
            token, arena, blk = kv_block
            seed = int(torch.randint(0, 2 ** 31 - 1, (1,)).item()) if pdrop > 0.0 else 0
            o = ops.attention_block(qp, k_proj, v_proj, token, arena, blk, h, pdrop, seed)
        else:
            o = _attn(qp, k_proj, v_proj, h, pdrop)
        tgt2 = _lin(o, ca.out_proj.weight, ca.out_proj.bias)
        tgt = _add_norm(tgt, tgt2, self.norm2, self.dropout2, self.training)
        if self.activation is not F.relu:
            raise RuntimeError("pointnet_refine_amd: the FFN activation is ReLU (src/model.py:95), fused into the GEMM epilogue")
        # linear2(dropout(relu(linear1(tgt)))) (src/model.py:131): ReLU AND the dropout ride on linear1's epilogue
        pd = self.dropout.p if self.training else 0.0
        seed = int(torch.randint(0, 2 ** 31 - 1, (1,)).item()) if pd > 0.0 else 0
        # hid's largest magnitude is a by-product of that epilogue: linear2 takes it instead of a read pass over hid
        hid, hid_amax = ops.linear_with_amax(tgt, self.linear1.weight, self.linear1.bias, None, True, None, pd, seed)
        tgt2 = ops.linear(hid, self.linear2.weight, self.linear2.bias, hid_amax)
        tgt = _add_norm(tgt, tgt2, self.norm3, self.dropout3, self.training)
        return tgt


class LineRefineNet(nn.Module):
    """Reference: src/model.py:137-234.  forward(context (B,N,4), noisy_line (B,M,3)) ->
    (6,B,M,3) cumulative offsets per decoder layer."""

    def __init__(self, num_line_points=32, feature_dim=1024):
        super().__init__()                         # num_line_points: accepted and unused, as in the reference
        d = self.d_model = 256
        L = self.num_decoder_layers = 6
        self.context_encoder = MultiScalePointNetEncoder(in_channel=4, out_dim=feature_dim)
        self.context_proj = nn.Linear(feature_dim, d)
        # line encoder 3 -> 64 -> 128 -> 256: conv+BN pairs, ReLU after the first two only
        # (Sequential indices 0/1, 3/4, 6/7 as in the reference's state_dict)
        stack, widths = [], (3, 64, 128, d)
        for k in range(1, 4):
            stack += [nn.Conv1d(widths[k - 1], widths[k], kernel_size=1), nn.BatchNorm1d(widths[k])]
            if k < 3:
                stack.append(nn.ReLU())
        self.point_mlp = nn.Sequential(*stack)
        self.pos_emb = PositionalEncoding(in_dim=3, out_dim=d)
        self.decoder_layers = nn.ModuleList(
            DetrTransformerDecoderLayer(d_model=d, nhead=8, dim_feedforward=1024) for _ in range(L))
        self.reg_branches = nn.ModuleList(
            nn.Sequential(nn.Linear(d, 128), nn.ReLU(), nn.Linear(128, 3)) for _ in range(L))

    # -- accelerated rows -------------------------------------------------------------------
    def encode_context(self, context, defer_check=False):
        """context (B,N,4) -> memory (B,N,256): encoder + context_proj (src/model.py:192-194).
        defer_check: the fused eval kernel's saturation counter is read by the caller after it has queued
        the rest of its work (LineRefineNet.forward), not here."""
        enc = self.context_encoder
        if context.dim() != 3:
            raise RuntimeError(f"Expected 3D (batched) input, but got input of size: {list(context.shape)}")
        if enc._fused_ok(context) and tuple(self.context_proj.weight.shape) == (256, 1024):
            # inference: encoder + context_proj as ONE kernel, no activation leaves the chip
            try:
                memory, _, _ = ops.encoder_eval_fused(context, enc._param_list(), enc._bn_buffer_list(), enc.bn1.eps,
                                                      self.context_proj.weight, self.context_proj.bias,
                                                      precision=enc.inference_precision, check=not defer_check)
                self._fused_pending = defer_check
                return memory
            except ops.FusedSaturation as e:
                _warn_saturated(e)
        _, fused, fused_amax = ops.encoder_with_amax(context, enc._param_list(), enc._bn_buffer_list(), False,
                                                     enc.training, enc.bn1.momentum, enc.bn1.eps)
        memory, mem_amax = ops.linear_with_amax(fused, self.context_proj.weight, self.context_proj.bias, fused_amax)
        ops.amax_note(memory, mem_amax)      # decode() hands it to the V projection and the positional residual's consumer
        return memory

    def encode_line(self, noisy_line):
        """noisy_line (B,M,3) -> initial queries (B,M,256): point_mlp (src/model.py:200-201)."""
        B, M, _ = noisy_line.shape
        pm = self.point_mlp
        layers = [(pm[0].weight, pm[0].bias, pm[1].weight, pm[1].bias),
                  (pm[3].weight, pm[3].bias, pm[4].weight, pm[4].bias),
                  (pm[6].weight, pm[6].bias, pm[7].weight, pm[7].bias)]
        buffers = _bn_buffers(pm[1]) + _bn_buffers(pm[4]) + _bn_buffers(pm[7])
        y = ops.mlp_stack(noisy_line.reshape(B * M, -1), layers, buffers, relu_last=False,
                          training=self.training, momentum=pm[1].momentum, eps=pm[1].eps)
        return y.reshape(B, M, -1)

    fold_kv_inference = True      # False: reduced-precision inference keeps the K / V projection GEMMs

    def _fold_ok(self, memory, noisy_line):
        """Folded cross-attention: eval mode without autograd, on the GPU, in the reduced-precision
        GEMM mode (io.refine_scene(precision="fp16"), bench --gemm bf16), reference widths."""
        return (self.fold_kv_inference and not self.training and not torch.is_grad_enabled() and memory.is_cuda
                and ops.bf16_mode() and self.d_model == 256 and noisy_line.shape[1] <= 32
                and self.decoder_layers[0].cross_attn.num_heads == 8)

    def decode(self, context, noisy_line, memory, tgt):
        """Iterative refinement (src/model.py:197-234) given memory (B,N,256) and the initial
        queries tgt (B,M,256).  No BatchNorm in here, so it may be run on batch chunks.

        Same arithmetic as the reference's decoder layers, reorganised around what is constant
        over the six layers: `memory` and `pos_mem` do not change, so the cross-attention key
        and value projections of ALL layers (src/model.py:123-126: k = memory+pos, v = memory,
        packed in_proj rows [256:512] and [512:768]) are two GEMMs of width 6*256 on the HIP
        GEMM cores instead of twelve library GEMMs plus six elementwise adds."""
        d = self.d_model
        layers = self.decoder_layers
        fold = self._fold_ok(memory, noisy_line)
        if fold:
            # reduced-precision inference (BASELINE config 5): no K / V projection at all - every
            # layer attends over the raw rows of memory + pos and memory with its projections
            # folded into the kernel (csrc/prh_attnfold.hpp).  The two bf16 row images are made
            # once, straight from the points and `memory` (the positional MLP runs inside that pass)
            l0, l2 = self.pos_emb.mlp[0], self.pos_emb.mlp[2]
            if tuple(l0.weight.shape) == (256, 3) and tuple(l2.weight.shape) == (256, 256):
                k_all, v_all = ops.posmem_images(context[:, :, :3], memory, l0.weight, l0.bias, l2.weight, l2.bias)
            else:
                mempos = self.pos_emb(context[:, :, :3], resid=memory)
                k_all, v_all = ops.cast_perm_bf16(mempos), ops.cast_perm_bf16(memory)
        # split-fp16 training path: pos_emb's second Linear and the two wide projections are ONE autograd node
        # that hands every operand maximum from its producer to its consumer (ops.PosKVFn)
        span = (not fold and ops.producer_maxima_on(memory.is_cuda) and memory.dtype == torch.float32
                and context.dtype == torch.float32)
        if not fold and not span:
            mempos = self.pos_emb(context[:, :, :3], resid=memory)      # memory + pos_mem, (B, N, 256)
        cat = ops.cat_rows
        if d != 256:
            raise RuntimeError("pointnet_refine_amd: the decoder kernels are built for d_model = 256 (src/model.py:141)")
        if not fold:
            wk = cat([l.cross_attn.in_proj_weight[d:2 * d] for l in layers])
            bk = cat([l.cross_attn.in_proj_bias[d:2 * d] for l in layers])
            wv = cat([l.cross_attn.in_proj_weight[2 * d:] for l in layers])
            bv = cat([l.cross_attn.in_proj_bias[2 * d:] for l in layers])
        if fold:
            pass
        elif span:
            h, h_amax = self.pos_emb.hidden(context[:, :, :3])
            l2 = self.pos_emb.mlp[2]
            k_all, v_all = ops.pos_kv_project(h, memory, l2.weight, l2.bias, wk, bk, wv, bv, h_amax,
                                              ops.amax_of(memory))       # (B, N, 6*256) each
        elif ops.bf16_mode() and mempos.is_cuda:
            # bf16 mode (BASELINE config 3): the wide K / V buffers and their gradients live in bf16
            k_all = ops.linear_out16(mempos, wk, bk)                # (B, N, 6*256) bf16
            v_all = ops.linear_out16(memory, wv, bv)
        else:
            k_all = ops.linear(mempos, wk, bk)                      # (B, N, 6*256)
            v_all = ops.linear(memory, wv, bv)
        if fold:
            token = arena = None
        else:
            # the fused attention kernels read column block i of k_all / v_all in place and
            # write dK / dV straight into one gradient buffer each (ops.GradArena): no
            # per-layer K/V tensors, no concatenation of their gradients
            token, arena = ops.kv_token(k_all, v_all, d)
        current_line_coords = noisy_line.clone()
        all_pred_offsets = []
        for i, (decoder_layer, reg_branch) in enumerate(zip(layers, self.reg_branches)):
            pos_tgt = self.pos_emb(current_line_coords)
            if fold:
                tgt = decoder_layer.forward_projected(tgt, k_all, v_all, query_pos=pos_tgt, kv_block=("fold", None, i))
            else:
                tgt = decoder_layer.forward_projected(tgt, k_all, v_all, query_pos=pos_tgt,
                                                      kv_block=(token, arena, i))
            r0, r2 = reg_branch[0], reg_branch[2]
            hid = ops.linear(tgt, r0.weight, r0.bias, None, True)                   # 256 -> 128, ReLU in the epilogue
            if not ops.linear_small_supported(r2.in_features, r2.out_features):
                raise RuntimeError(f"pointnet_refine_amd: regression head Linear({r2.in_features}, {r2.out_features}) "
                                   "is not supported by the one-pass kernel")
            delta_offset = ops.linear_small(hid, r2.weight, r2.bias)                # 128 -> 3: one HBM pass
            current_line_coords = current_line_coords + delta_offset      # no detach (H5)
            all_pred_offsets.append(current_line_coords - noisy_line)
        return torch.stack(all_pred_offsets)

    def forward(self, context, noisy_line):
        if context.dim() != 3 or noisy_line.dim() != 3:
            raise RuntimeError("LineRefineNet expects context (B,N,4) and noisy_line (B,M,3)")
        self._fused_pending = False
        memory = self.encode_context(context, defer_check=True)     # (B, N, 256)
        tgt = self.encode_line(noisy_line)                          # (B, M, 256)
        out = self.decode(context, noisy_line, memory, tgt)
        if self._fused_pending:
            # the fused eval kernel ran: read its saturation counter now that the whole forward is queued
            # (one 4-byte copy; the caller is about to read `out` anyway) and redo the call on the
            # per-layer kernels if an activation left the fp16 range
            self._fused_pending = False
            n = ops.fused_saturation(context.device)
            if n:
                _warn_saturated(ops.FusedSaturation(f"{n} activation groups exceeded the fp16 range in the fused eval kernel"))
                enc, old = self.context_encoder, self.context_encoder.inference_precision
                enc.inference_precision = None
                try:
                    memory = self.encode_context(context)
                    out = self.decode(context, noisy_line, memory, tgt)
                finally:
                    enc.inference_precision = old
        return out
