"""The W8A16 GEMM above 64 rows (csrc/gemm_w8_rows.hip) and the executor route onto it, on the GPU.

SHAPES x TS are the issue's cases.  Rows: one past 64 (the narrow geometry, a 1-row second wave), one past a
128-row block, one past two, and 300 (a last block of 44 rows whose last row tile is partial).  On 256 CUs
the column split cuts every one of those shapes into groups of ONE unit (there are fewer column tiles than
CUs per row block), so only the last column wave of a workgroup computes, on its tile slot 0.  FULL adds the
cases whose groups fill a geometry, as the model shapes do (units > capacity x CUs / row blocks), at K = 128:

  wide (T = 2049: 17 row blocks, 16 tiles a group at most)
    N 4096 / 8192 SwiGLU   16 groups of 16 tiles / 32 of 8 pairs: every wave 4 tiles, slots 0..3, u0 = 0, 4, 8, 12
    N 4000 / 8000 SwiGLU   groups of 16 and 15 tiles / 8 and 7 pairs (NBB != NBS): waves of 3 and 4 tiles / 1 and 2 pairs
  narrow (T = 65: 4 tiles a group at most)
    N 16384, both          256 groups of 4 tiles / 2 pairs: both column waves 2 tiles
    N 16000                groups of 4 and 3 tiles: waves of 1 and 2 tiles

Weights and references are made once per shape.
"""
import functools

import pytest
import torch

from src import ops
from src.models.config import resolve_model
from src.models.reference_model import reference_forward
from src.models.weights import random_stage_weights
from src.ops.reference import GU_BLOCK
from src.runtime.executor import StageExecutor

from .test_moe_fp8 import dequantized
from .test_moe_fp8_gpu import _fp8_mixtral, rows
from .test_moe_rows_gpu import check

pytestmark = pytest.mark.gpu
DEV = "cuda"
SHAPES = [(768, 512, 0), (560, 512, 0), (512, 1024, 0), (1152, 2304, 0), (2048, 512, 1), (4608, 1024, 1)]
TS = [65, 129, 257, 300]
FULL = [(4096, 128, 0, 2049), (8192, 128, 1, 2049), (4000, 128, 0, 2049), (8000, 128, 1, 2049),
        (16384, 128, 0, 65), (16384, 128, 1, 65), (16000, 128, 0, 65)]
CASES = [s + (T,) for s in SHAPES for T in TS] + FULL
SENTINEL = 7.0


@functools.lru_cache(maxsize=None)
def weight(N, K):
    """(w8, scales, fp64 dequantized [N, K]); w ~ 0.02 N(0, 1)."""
    g = torch.Generator(device=DEV).manual_seed(N * 31 + K)
    q, s = ops.pack_weight_fp8(0.02 * torch.randn(N, K, device=DEV, generator=g))
    w8 = ops.w8_from_fp8(q)
    return w8, s, ops.unpack_weight_w8(w8, s, torch.float64)


def oracle(x, wd, epi):
    y = x.double() @ wd.t()
    if epi == 1:
        g, u = y.view(x.shape[0], -1, 2, GU_BLOCK).unbind(2)
        y = (g * torch.sigmoid(g) * u).reshape(x.shape[0], -1)
    return y


@pytest.mark.parametrize("N,K,epi,T", CASES)
def test_matches_the_fp64_reference_repeats_bit_for_bit_and_stays_inside_out(N, K, epi, T):
    assert ops.w8_rows_ok(T, N, K, epi)
    w8, ws, wd = weight(N, K)
    x, nc = rows(T, K, T), N // 2 if epi else N
    buf = torch.full((T + 3, nc + 24), SENTINEL, dtype=torch.bfloat16, device=DEV)
    out = buf[:T, 8:8 + nc]
    assert ops.linear_w8_rows(x, w8, ws, out=out, epilogue=epi) is out
    check(out, oracle(x, wd, epi), f"N={N} K={K} epilogue={epi} T={T}")
    assert torch.equal(ops.linear_w8_rows(x, w8, ws, epilogue=epi), out)
    inside = torch.zeros_like(buf, dtype=torch.bool)
    inside[:T, 8:8 + nc] = True
    assert bool((buf[~inside] == SENTINEL).all())


@pytest.mark.parametrize("N,K,epi,T", [s + (T,) for s in [(560, 512, 0), (2048, 512, 1)] for T in TS] + FULL[2:4])
def test_strided_input_and_isolated_rows(N, K, epi, T):
    w8, ws, _ = weight(N, K)
    x = rows(T, K, T)
    y = ops.linear_w8_rows(x, w8, ws, epilogue=epi)
    wide = torch.full((T, K + 64), float("nan"), dtype=torch.bfloat16, device=DEV)
    wide[:, :K] = x
    assert wide[:, :K].stride(0) == K + 64
    assert torch.equal(ops.linear_w8_rows(wide[:, :K], w8, ws, epilogue=epi), y)
    for r in (64, T - 1):
        xn = x.clone()
        xn[r] = float("nan")
        yn = ops.linear_w8_rows(xn, w8, ws, epilogue=epi)
        keep = torch.arange(T, device=DEV) != r
        assert not torch.isfinite(yn[r].float()).any()
        assert torch.equal(yn[keep], y[keep])


def test_uncovered_shapes_and_bad_arguments_launch_nothing():
    assert ops.w8_rows_ok(65, 768, 512, 0) and ops.w8_rows_ok(1 << 20, 48, 128, 0)
    assert not ops.w8_rows_ok(64, 768, 512, 0) and not ops.w8_rows_ok(65, 768, 96, 0)
    assert not ops.w8_rows_ok(65, 48, 512, 1)
    w8, ws, _ = weight(768, 512)
    x = rows(65, 512, 1)
    out = torch.full((65, 768), SENTINEL, dtype=torch.bfloat16, device=DEV)
    with pytest.raises(RuntimeError, match="x must be bf16"):
        torch.ops.mpamd.gemm_w8_rows(x.half(), w8, ws, out, 0)
    with pytest.raises(RuntimeError, match="w_scale"):
        torch.ops.mpamd.gemm_w8_rows(x, w8, ws.double(), out, 0)
    with pytest.raises(RuntimeError, match="out must be"):
        torch.ops.mpamd.gemm_w8_rows(x, w8, ws, out[:, :384], 0)
    with pytest.raises(ValueError, match="out must be"):
        ops.linear_w8_rows(x, w8, ws, out=out[:64])
    odd = torch.zeros(65, 516, dtype=torch.bfloat16, device=DEV)[:, :512]
    with pytest.raises(RuntimeError, match="x needs"):
        torch.ops.mpamd.gemm_w8_rows(odd, w8, ws, out, 0)
    with pytest.raises(ValueError, match="x must have"):
        ops.linear_w8_rows(odd, w8, ws, out=out)
    with pytest.raises(RuntimeError, match="no kernel covers"):
        torch.ops.mpamd.gemm_w8_rows(x[:64], w8, ws, out[:64], 0)
    torch.cuda.synchronize()
    assert bool((out == SENTINEL).all())


# ------------------------------------------------------------------ executor
def _fp8_llama(seed=4):
    cfg = resolve_model("small-llama")
    mk = lambda **kw: random_stage_weights(cfg, 0, cfg.num_hidden_layers, has_embed=True, has_head=True,  # noqa: E731
                                           device=DEV, dtype=torch.bfloat16, seed=seed, **kw)
    return cfg, mk, dequantized(mk(), torch.float32)


@pytest.mark.parametrize("env,prefill,decode", [({}, True, False), ({"MPAMD_W8_ROWS_DECODE": "1"}, True, True),
                                                ({"MPAMD_W8_ROWS": "0", "MPAMD_W8_ROWS_DECODE": "1"}, False, False)])
@pytest.mark.parametrize("model,per_layer", [(_fp8_llama, 4), (_fp8_mixtral, 2)])
def test_fp8_steps_above_64_rows_read_the_weights_in_place(model, per_layer, env, prefill, decode, monkeypatch):
    """An 80 + 9-token prefill and a 65-session decode step against the fp32 oracle over the dequantized
    weights (the fp8 executor tests' bound).  Prefill steps take ops.linear_w8_rows for every W8A16
    projection by default; a pure decode step keeps its recorded launches (tests/golden/executor_paths)
    unless MPAMD_W8_ROWS_DECODE=1; MPAMD_W8_ROWS=0 is the dequantizing schedule everywhere.  Graphs stop at 64
    sessions on both stages (an fp8 Mixtral stage's own limit): every step here runs eagerly, once."""
    cfg, mk, oracle_w = model()
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    calls = [0]

    def counted(*a, _f=ops.linear_w8_rows, **kw):
        calls[0] += 1
        return _f(*a, **kw)

    monkeypatch.setattr(ops, "linear_w8_rows", counted)
    ex = StageExecutor(cfg, mk(quant_type="fp8"), DEV, kv_cache_bytes=128 << 20, max_sessions=80, max_seq_len=128,
                       use_graphs=True, graph_max_batch=64, warmup=False)
    per_step = per_layer * cfg.num_hidden_layers
    g = torch.Generator().manual_seed(3)
    prompts = [torch.randint(0, cfg.vocab_size, (n,), generator=g) for n in (80, 9)]
    logits = ex.forward([("a", 80), ("b", 9)], torch.cat(prompts).cuda())
    assert calls[0] == (per_step if prefill else 0)
    for i, p in enumerate(prompts):
        torch.testing.assert_close(logits[i].float(), reference_forward([oracle_w], p.cuda())[-1], atol=0.06, rtol=0.05)
    n, plen = 65, 3
    ids = torch.randint(0, cfg.vocab_size, (n, plen), generator=g)
    nxt = torch.argmax(ex.forward([(f"s{i}", plen) for i in range(n)], ids.reshape(-1).cuda()).float(), -1)
    before = calls[0]
    logits = ex.forward([(f"s{i}", 1) for i in range(n)], nxt)
    assert calls[0] == before + (per_step if decode else 0)
    for i in (0, 64):
        seq = torch.cat([ids[i], nxt[i:i + 1].cpu()]).cuda()
        torch.testing.assert_close(logits[i].float(), reference_forward([oracle_w], seq)[-1], atol=0.06, rtol=0.05)
