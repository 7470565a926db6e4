"""The fp64 attention reference of tests/_attn_ref.py checked against torch's own operators, on the CPU: the GPU tests
of the attention kernels (tests/test_attn_variants_gpu.py) are only as good as this reference."""
import pytest
import torch

import _attn_ref as R


def _operands(B, H, M, N, seed):
    C = 32 * H
    g = torch.Generator().manual_seed(seed)
    q = torch.randn(B, M, C, generator=g, dtype=torch.float64)
    k = torch.randn(B, N, C, generator=g).to(torch.bfloat16).double()
    v = torch.randn(B, N, C, generator=g).to(torch.bfloat16).double()
    up = torch.randn(B, M, C, generator=g, dtype=torch.float64)
    return q, k, v, up


@pytest.mark.parametrize("B,H,M,N", [(2, 8, 32, 33), (1, 4, 45, 70), (2, 12, 20, 1)])
def test_attn_ref_matches_sdpa_and_logsumexp(B, H, M, N):
    q, k, v, _ = _operands(B, H, M, N, 1)
    scale = 32.0 ** -0.5
    o, lse = R.attn_ref(q, k, v, H, scale)
    hd = lambda x: x.view(B, -1, H, 32).transpose(1, 2)
    sd = torch.nn.functional.scaled_dot_product_attention(hd(q), hd(k), hd(v), scale=scale)
    sd = sd.transpose(1, 2).reshape(B, M, 32 * H)
    assert float((o - sd).abs().max()) < 1e-12
    ref_lse = torch.logsumexp(hd(q) @ hd(k).transpose(-1, -2) * scale, dim=-1)
    assert lse.shape == (B, H, M) and float((lse - ref_lse).abs().max()) < 1e-13


@pytest.mark.parametrize("B,H,M,N,p", [(2, 8, 32, 33, 0.0), (1, 8, 70, 40, 0.0), (2, 4, 45, 70, 0.2)])
def test_tile_contributions_sum_to_the_one_shot_gradient(B, H, M, N, p):
    from pointnet_refine_amd import ops
    q, k, v, up = _operands(B, H, M, N, 2)
    scale = 32.0 ** -0.5
    keep = ops.attention_keep_mask(B, H, M, N, p, 77, device="cpu") if p > 0 else None
    dq, ck, cv = R.attn_grads_ref(q, k, v, up, H, scale, keep, p)
    assert len(ck) == len(cv) == (M + R.QT - 1) // R.QT
    q1, k1, v1 = (t.clone().requires_grad_(True) for t in (q, k, v))
    o, _ = R.attn_ref(q1, k1, v1, H, scale, keep, p)
    (o * up).sum().backward()
    for got, want in ((dq, q1.grad), (ck[-1], k1.grad), (cv[-1], v1.grad)):
        assert float((got - want).norm() / want.norm()) < 1e-12
    if len(ck) > 1:      # the running sums are not the total all along
        assert float((ck[0] - ck[-1]).norm()) > 1e-3 * float(ck[-1].norm())


def test_dropout_matches_the_written_out_formula():
    """attn_ref with the kernels' keep-mask against the reference formula of tests/test_attention_gpu.py."""
    from pointnet_refine_amd import ops
    from test_attention_gpu import _ref
    B, H, M, N, p = 2, 8, 45, 70, 0.2
    q, k, v, _ = _operands(B, H, M, N, 3)
    keep = ops.attention_keep_mask(B, H, M, N, p, 1234567, device="cpu")
    assert 0.7 < float(keep.double().mean()) < 0.9
    o, lse = R.attn_ref(q, k, v, H, 32.0 ** -0.5, keep, p)
    assert float((o - _ref(q, k, v, H, keep, p)).abs().max()) < 1e-12
    o0, lse0 = R.attn_ref(q, k, v, H, 32.0 ** -0.5)
    assert torch.equal(lse, lse0) and float((o - o0).abs().max()) > 1e-2      # lse is taken before dropout


def test_bf16_store_bound_is_one_rounding_for_one_tile():
    c = [torch.tensor([1.0, -3.0, 0.0], dtype=torch.float64)]
    b = R.bf16_store_bound(c)
    assert torch.allclose(b, 1.05 * 2.0 ** -8 * c[0].abs() + 2e-5 * 3.0, rtol=0, atol=1e-15)
    x = torch.randn(4096, dtype=torch.float64)
    assert bool(((x.to(torch.bfloat16).double() - x).abs() <= 2.0 ** -8 * x.abs()).all())
