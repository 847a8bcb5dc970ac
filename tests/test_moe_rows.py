"""Row-gathered grouped MoE ops (ops.moe_group / moe_gate_up_w8_rows / moe_down_w8_rows) - the torch
forms CPU executors run: the grouping against the stable argsort, and the three composed against
``moe.moe_mlp_torch`` over the dequantized weights.  The kernels: tests/test_moe_rows_gpu.py.
"""
import pytest
import torch

from src import ops
from src.ops import moe


@pytest.mark.parametrize("T,E,k", [(5, 4, 2), (70, 8, 2), (33, 4, 1)])
def test_group_equals_the_stable_argsort(T, E, k):
    g = torch.Generator().manual_seed(T)
    w, idx = moe.route(torch.randn(T, E, generator=g), k)
    off, tok, wsel = ops.moe_group(idx, w, E)
    order = torch.argsort(idx.reshape(-1), stable=True)
    assert off.dtype == tok.dtype == torch.int32 and off.shape == (E + 1,)
    assert off.tolist() == [0] + torch.cumsum(torch.bincount(idx.reshape(-1), minlength=E), 0).tolist()
    assert torch.equal(tok, (order // k).int()) and torch.equal(wsel, w.reshape(-1)[order])


@pytest.mark.parametrize("T", [3, 70])
def test_torch_forms_compose_to_the_moe_mlp(T):
    H, F, E, k = 256, 128, 4, 2
    g = torch.Generator().manual_seed(7)
    x = torch.randn(T, H, generator=g)
    router = torch.randn(E, H, generator=g)
    quant = lambda w: [ops.pack_weight_fp8(w[e]) for e in range(E)]  # noqa: E731
    gu, dn = quant(0.02 * torch.randn(E, 2 * F, H, generator=g)), quant(0.02 * torch.randn(E, H, F, generator=g))
    gu8, gus = torch.stack([ops.w8_from_fp8(q) for q, _ in gu]), torch.stack([s for _, s in gu])
    dn8, dns = torch.stack([ops.w8_from_fp8(q) for q, _ in dn]), torch.stack([s for _, s in dn])
    w, idx = moe.route(x @ router.t(), k)
    off, tok, wsel = ops.moe_group(idx, w, E)
    act = ops.moe_gate_up_w8_rows(x, gu8, gus, off, tok)
    y = ops.moe_down_w8_rows(act, dn8, dns, off, tok, wsel, T)
    want = moe.moe_mlp_torch(x, router, torch.stack([ops.unpack_weight_fp8(q, s, torch.float32) for q, s in gu]),
                             torch.stack([ops.unpack_weight_fp8(q, s, torch.float32) for q, s in dn]), k)
    assert act.shape == (T * k, F) and y.shape == (T, H)
    torch.testing.assert_close(y, want, atol=1e-5, rtol=1e-4)
    with pytest.raises(ValueError, match="off"):
        ops.moe_gate_up_w8_rows(x, gu8, gus, off[:-1], tok)
    with pytest.raises(ValueError, match="act"):
        ops.moe_down_w8_rows(act[:-1], dn8, dns, off, tok, wsel, T)
