"""Tiled grouped MoE ops (ops.moe_gate_up_w8_tiled / moe_down_w8_tiled / moe_combine_tiled) - the torch forms
CPU tensors take: equal to the row-gathered ops' torch forms to fp32 round-off, and the per-pair slot rule
j = #{valid ids < e} with an expert id out of range.  The kernels: tests/test_moe_tiled_gpu.py.
"""
import torch

from src import ops

H, F, E = 256, 128, 4


def edge_routing(T=258, device="cpu"):
    """tokens 0..127 -> (0, 3), 128..256 -> (1, 3), 257 -> (2, 3): counts 128, 129, 1, 258."""
    t = torch.arange(T, device=device)
    idx = torch.stack([(t >= 128).long() + (t >= 257).long(), torch.full_like(t, 3)], 1)
    g = torch.Generator().manual_seed(T)
    return idx, torch.softmax(torch.randn(T, 2, generator=g), -1).to(device)


def weights():
    g = torch.Generator().manual_seed(7)
    stacks = []
    for N, K in ((2 * F, H), (H, F)):
        q = [ops.pack_weight_fp8(0.02 * torch.randn(N, K, generator=g)) for _ in range(E)]
        stacks += [torch.stack([ops.w8_from_fp8(c) for c, _ in q]), torch.stack([s for _, s in q])]
    return stacks


def test_torch_forms_equal_the_row_gathered_forms_on_the_edge_routing():
    gu8, gus, dn8, dns = weights()
    idx, w = edge_routing()
    T = idx.shape[0]
    off, tok, wsel = ops.moe_group(idx, w, E)
    assert off.tolist() == [0, 128, 257, 258, 516]
    x = torch.randn(T, H, generator=torch.Generator().manual_seed(1))
    act = ops.moe_gate_up_w8_tiled(x, gu8, gus, off, tok)
    assert torch.equal(act, ops.moe_gate_up_w8_rows(x, gu8, gus, off, tok))
    y = ops.moe_down_w8_tiled(act, dn8, dns, off, tok, wsel, idx, T)
    torch.testing.assert_close(y, ops.moe_down_w8_rows(act, dn8, dns, off, tok, wsel, T), atol=1e-6, rtol=1e-5)


def test_a_pair_with_an_expert_id_out_of_range_is_dropped_and_the_other_pair_lands():
    """Token 1 is routed to (E, 0) and token 2 to (-1, 3): the grouping drops those pairs (off[E] < T k), the
    valid pair takes slot 0 of its token and the combine reads that slot alone."""
    gu8, gus, dn8, dns = weights()
    T = 4
    idx = torch.tensor([[1, 2], [E, 0], [-1, 3], [0, 3]])
    w = torch.full((T, 2), 0.5)
    flat = idx.reshape(-1)
    keep = torch.nonzero((flat >= 0) & (flat < E)).squeeze(1)
    order = keep[torch.argsort(flat[keep], stable=True)]
    off = torch.zeros(E + 1, dtype=torch.int32)
    off[1:] = torch.cumsum(torch.bincount(flat[keep], minlength=E), 0)
    tok = torch.zeros(2 * T, dtype=torch.int32)
    wsel = torch.zeros(2 * T)
    tok[:order.numel()], wsel[:order.numel()] = (order // 2).int(), w.reshape(-1)[order]
    act = torch.randn(2 * T, F, generator=torch.Generator().manual_seed(2))
    y = ops.moe_down_w8_tiled(act, dn8, dns, off, tok, wsel, idx, T)
    assert torch.isfinite(y).all()
    want = torch.zeros(T, H)
    for p in range(int(off[E])):
        e = int(torch.searchsorted(off[1:], p, right=True))
        want[tok[p]] += wsel[p] * (act[p] @ ops.unpack_weight_w8(dn8[e], dns[e], torch.float32).t())
    torch.testing.assert_close(y, want, atol=1e-6, rtol=1e-5)
    assert y[1].abs().max() > 0 and y[2].abs().max() > 0
