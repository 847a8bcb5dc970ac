"""The W4A16 GEMM above 64 rows (csrc/gemm_w4_rows.hip) and the executor route onto it, on the GPU.

Weights: 0.02 N(0, 1) with every 32-wide k-block of every row multiplied by 2^j, j uniform in -6 .. 6, so
neighbouring k-slices and neighbouring columns carry e8m0 bytes many binades apart: a slice that took another
slice's or another column's scale is a gross error, not a rounding difference.  The oracle is the fp64
product with the torch dequantization of the same codes.

SHAPES x TS: one stage (K = 128: the prologue and one step), 35 tiles x three stages (odd both), and the rows
one past 64, one past one and two 128-row blocks, and 300 (a last block whose last row tile is partial).  FULL
is tests/test_w8_rows_gpu.py's list - the cases whose column groups fill a geometry on 256 CUs; its docstring
says why.  Weights are made once per shape.
"""
import functools

import pytest
import torch

from src import ops
from src.models.reference_model import reference_forward
from src.ops import reference as ref
from src.ops.reference import GU_BLOCK
from src.runtime.executor import StageExecutor

from .test_moe_fp8_gpu import rows
from .test_moe_rows_gpu import check
from .test_mxfp4_gpu import _check_oracle, w4_stage  # noqa: F401  (w4_stage: a fixture)

pytestmark = pytest.mark.gpu
DEV = "cuda"
SHAPES = [(768, 128, 0), (560, 384, 0), (512, 1024, 0), (2048, 256, 1), (4608, 512, 1)]
TS = [65, 129, 257, 300]
FULL = [(4096, 128, 0, 2049), (8192, 128, 1, 2049), (4000, 128, 0, 2049), (8000, 128, 1, 2049),
        (16384, 128, 0, 65), (16384, 128, 1, 65), (16000, 128, 0, 65)]
CASES = [s + (T,) for s in SHAPES for T in TS] + FULL
SENTINEL = 7.0


@functools.lru_cache(maxsize=None)
def weight(N, K):
    """(w4, s4, fp64 dequantized [N, K])."""
    g = torch.Generator(device=DEV).manual_seed(N * 31 + K)
    w = 0.02 * torch.randn(N, K, device=DEV, generator=g)
    j = torch.randint(-6, 7, (N, K // 32), device=DEV, generator=g)
    w4, s4 = ops.pack_weight_w4(w * torch.exp2(j.float()).repeat_interleave(32, 1))
    return w4, s4, ref.unpack_weight_w4(w4, s4, torch.float64)


def oracle(x, wd, epi):
    y = x.double() @ wd.t()
    if epi == 1:
        g, u = y.view(x.shape[0], -1, 2, GU_BLOCK).unbind(2)
        y = (g * torch.sigmoid(g) * u).reshape(x.shape[0], -1)
    return y


@pytest.mark.parametrize("N,K,epi,T", CASES)
def test_matches_the_fp64_reference_repeats_bit_for_bit_and_stays_inside_out(N, K, epi, T):
    assert ops.w4_rows_ok(T, N, K, epi)
    w4, s4, wd = weight(N, K)
    x, nc = rows(T, K, T), N // 2 if epi else N
    buf = torch.full((T + 3, nc + 24), SENTINEL, dtype=torch.bfloat16, device=DEV)
    out = buf[:T, 8:8 + nc]
    assert ops.linear_w4_rows(x, w4, s4, out=out, epilogue=epi) is out
    want = oracle(x, wd, epi)
    check(out, want, f"N={N} K={K} epilogue={epi} T={T}")
    if epi == 0:  # half a bf16 ulp, doubled, plus a worst-case fp32 sum of K terms
        bound = 2.0 ** -8 * want.abs() + K * 2.0 ** -22 * (x.double().abs() @ wd.abs().t())
        excess = ((out.double() - want).abs() - bound).max()
        print(f"largest |y - want| - bound: {float(excess):.3g}")
        assert float(excess) <= 0
    assert torch.equal(ops.linear_w4_rows(x, w4, s4, epilogue=epi), out)
    inside = torch.zeros_like(buf, dtype=torch.bool)
    inside[:T, 8:8 + nc] = True
    assert bool((buf[~inside] == SENTINEL).all())


@pytest.mark.parametrize("N,K,epi,T", [s + (T,) for s in [(560, 384, 0), (2048, 256, 1)] for T in TS] + FULL[2:4])
def test_strided_input_and_isolated_rows(N, K, epi, T):
    w4, s4, _ = weight(N, K)
    x = rows(T, K, T)
    y = ops.linear_w4_rows(x, w4, s4, epilogue=epi)
    wide = torch.full((T, K + 64), float("nan"), dtype=torch.bfloat16, device=DEV)
    wide[:, :K] = x
    assert wide[:, :K].stride(0) == K + 64
    assert torch.equal(ops.linear_w4_rows(wide[:, :K], w4, s4, epilogue=epi), y)
    for r in (64, T - 1):
        xn = x.clone()
        xn[r] = float("nan")
        yn = ops.linear_w4_rows(xn, w4, s4, epilogue=epi)
        keep = torch.arange(T, device=DEV) != r
        assert not torch.isfinite(yn[r].float()).any()
        assert torch.equal(yn[keep], y[keep])


def test_uncovered_shapes_and_bad_arguments_launch_nothing():
    assert ops.w4_rows_ok(65, 768, 128, 0) and ops.w4_rows_ok(1 << 20, 48, 128, 0)
    assert not ops.w4_rows_ok(64, 768, 128, 0) and not ops.w4_rows_ok(65, 768, 96, 0)
    assert not ops.w4_rows_ok(65, 48, 128, 1)
    w4, s4, _ = weight(768, 128)
    x = rows(65, 128, 1)
    out = torch.full((65, 768), SENTINEL, dtype=torch.bfloat16, device=DEV)
    with pytest.raises(RuntimeError, match="x must be bf16"):
        torch.ops.mpamd.gemm_w4_rows(x.half(), w4, s4, out, 0)
    with pytest.raises(RuntimeError, match="s4 must be"):
        torch.ops.mpamd.gemm_w4_rows(x, w4, s4[:-1], out, 0)
    with pytest.raises(RuntimeError, match="out must be"):
        torch.ops.mpamd.gemm_w4_rows(x, w4, s4, out[:, :384], 0)
    with pytest.raises(ValueError, match="out must be"):
        ops.linear_w4_rows(x, w4, s4, out=out[:64])
    odd = torch.zeros(65, 132, dtype=torch.bfloat16, device=DEV)[:, :128]
    with pytest.raises(RuntimeError, match="x needs"):
        torch.ops.mpamd.gemm_w4_rows(odd, w4, s4, out, 0)
    with pytest.raises(ValueError, match="x must have"):
        ops.linear_w4_rows(odd, w4, s4, out=out)
    with pytest.raises(RuntimeError, match="no kernel covers"):
        torch.ops.mpamd.gemm_w4_rows(x[:64], w4, s4, out[:64], 0)
    torch.cuda.synchronize()
    assert bool((out == SENTINEL).all())


# ------------------------------------------------------------------ executor
@pytest.mark.parametrize("env,prefill,decode", [
    ({"MPAMD_W4_ROWS": "4096"}, True, False),
    ({"MPAMD_W4_ROWS": "4096", "MPAMD_W4_ROWS_DECODE": "1"}, True, True),
    ({"MPAMD_W4_ROWS": "0", "MPAMD_W4_ROWS_DECODE": "1"}, False, False)])
def test_mxfp4_steps_above_64_rows_read_the_weights_in_place(w4_stage, env, prefill, decode, monkeypatch):  # noqa: F811
    """An 80 + 9-token prefill and a 65-session decode step against the fp32 oracle over the dequantized
    weights (the 4-bit executor tests' bound).  With a cap, prefill steps take ops.linear_w4_rows for all four
    projections of a layer; a pure decode step keeps its recorded launches (tests/golden/executor_paths)
    unless MPAMD_W4_ROWS_DECODE=1; MPAMD_W4_ROWS=0 is the dequantizing schedule everywhere."""
    cfg, w, wd = w4_stage
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    calls = [0]

    def counted(*a, _f=ops.linear_w4_rows, **kw):
        calls[0] += 1
        return _f(*a, **kw)

    monkeypatch.setattr(ops, "linear_w4_rows", counted)
    ex = StageExecutor(cfg, w, DEV, kv_cache_bytes=128 << 20, max_sessions=80, max_seq_len=128, use_graphs=False)
    per_step = 4 * cfg.num_hidden_layers
    g = torch.Generator().manual_seed(3)
    prompts = [torch.randint(0, cfg.vocab_size, (n,), generator=g) for n in (80, 9)]
    logits = ex.forward([("a", 80), ("b", 9)], torch.cat(prompts).cuda())
    assert calls[0] == (per_step if prefill else 0)
    _check_oracle(wd, [logits.float()], prompts, (0, 1))
    n, plen = 65, 3
    ids = torch.randint(0, cfg.vocab_size, (n, plen), generator=g)
    nxt = torch.argmax(ex.forward([(f"s{i}", plen) for i in range(n)], ids.reshape(-1).cuda()).float(), -1)
    before = calls[0]
    logits = ex.forward([(f"s{i}", 1) for i in range(n)], nxt)
    assert calls[0] == before + (per_step if decode else 0)
    _check_oracle(wd, [logits.float()], [torch.cat([ids[i], nxt[i:i + 1].cpu()]) for i in range(n)], (0, 64))
