"""``ops.lora_update_rows`` without a GPU: the torch fallback (row by row, the form ``ops.lora_expand`` uses)
against the update by runs, and the argument checks it shares with the decode ops."""
import pytest
import torch

from src import ops


def _case(T=97, K=352, N=528, R=48, S=4):
    g = torch.Generator().manual_seed(0)
    A = (torch.randn(S, R, K, generator=g) * K ** -0.5).bfloat16()
    B = (torch.randn(S, N, R, generator=g) * R ** -0.5).bfloat16()
    scale = torch.tensor([2.0, 0.5, 1.0, 16 / 8 ** 0.5])
    x, y = torch.randn(T, K, generator=g).bfloat16(), torch.randn(T, N, generator=g).bfloat16()
    sl = torch.tensor([(0, -1, 3, 1, -1)[(m // 9) % 5] for m in range(T)], dtype=torch.int32)  # runs of 9 rows
    return A, B, scale, x, y, sl


def test_the_fallback_equals_the_update_by_runs_and_leaves_base_rows_alone():
    A, B, scale, x, y0, sl = _case()
    xq = x.clone()
    xq[sl < 0] = float("nan")  # base rows are not read
    t = torch.full((x.shape[0], A.shape[1]), float("nan"))
    y = ops.lora_update_rows(xq, y0.clone(), A, B, scale, sl, t=t)
    want = ops.lora_update(xq, y0.clone(), A, B, scale, ops.lora_runs(sl.tolist()))
    base = sl < 0  # rows without an adapter: neither t nor y written
    assert torch.equal(y[base], y0[base]) and bool(torch.isnan(t[base]).all())
    assert not bool(torch.isnan(t[~base]).any()) and not torch.equal(y[~base], y0[~base])
    # one bf16 ulp of y: 2^-7 relative (8 significand bits), taken at the larger of the two results
    ulp = 2.0 ** -7 * torch.maximum(y.float().abs(), want.float().abs())
    assert bool(((y.float() - want.float()).abs() <= ulp).all())
    assert ops.lora_rows_ok(97, 528, 352, 48) and not ops.lora_rows_ok(97, 24, 352, 48)


def test_argument_checks_are_those_of_the_decode_ops():
    A, B, scale, x, y, sl = _case()
    T = x.shape[0]
    for bad in (sl.long(), sl[:5], sl.to("meta")):  # dtype, length, device
        with pytest.raises(ValueError, match="slots"):
            ops.lora_update_rows(x, y, A, B, scale, bad)
    with pytest.raises(ValueError, match="t must be"):
        ops.lora_update_rows(x, y, A, B, scale, sl, t=torch.zeros(T, 16))
    with pytest.raises(ValueError, match="scale"):
        ops.lora_update_rows(x, y, A, B, scale[:2], sl)
    with pytest.raises(ValueError, match="y must be"):  # a row stride that is no multiple of 8
        ops.lora_update_rows(x, torch.zeros(T, 532).bfloat16()[:, :528], A, B, scale, sl)
    with pytest.raises(ValueError, match="x must be"):
        ops.lora_update_rows(x[:, :320], y, A, B, scale, sl)
