"""The W8A8-MX GEMM above 64 rows (csrc/gemm_mx_rows.hip: quantizer + block-scaled MFMA GEMM) and the
executor route onto it, on the GPU.

The shapes are test_w8_rows_gpu.py's (its docstring says which geometry and split each one reaches), with
K = 384 for an odd number of k-stages.  The reference multiplies ops.mx_block_quant(x), the exact values the
quantizer produces, in fp64: what is left is fp32 summation order and one bf16 rounding.
"""
import dataclasses

import pytest
import torch

from src import ops
from src.models.config import resolve_model
from src.models.weights import random_stage_weights
from src.runtime.executor import StageExecutor

from .test_moe_fp8_gpu import rows
from .test_moe_rows_gpu import check
from .test_w8_rows_gpu import DEV, FULL, SENTINEL, TS, oracle, weight

pytestmark = pytest.mark.gpu
SHAPES = [(768, 512, 0), (560, 512, 0), (512, 384, 0), (1152, 2304, 0), (2048, 512, 1), (4608, 1024, 1)]
CASES = [s + (T,) for s in SHAPES for T in TS] + FULL


@pytest.mark.parametrize("N,K,epi,T", CASES)
def test_matches_the_fp64_reference_repeats_bit_for_bit_and_stays_inside_out(N, K, epi, T):
    assert ops.mx_rows_ok(T, N, K, epi)
    w8, ws, wd = weight(N, K)
    x, nc = rows(T, K, T), N // 2 if epi else N
    buf = torch.full((T + 3, nc + 24), SENTINEL, dtype=torch.bfloat16, device=DEV)
    out = buf[:T, 8:8 + nc]
    assert ops.linear_mx_rows(x, w8, ws, out=out, epilogue=epi) is out
    check(out, oracle(ops.mx_block_quant(x.float()), wd, epi), f"N={N} K={K} epilogue={epi} T={T}")
    assert torch.equal(ops.linear_mx_rows(x, w8, ws, epilogue=epi), out)
    inside = torch.zeros_like(buf, dtype=torch.bool)
    inside[:T, 8:8 + nc] = True
    assert bool((buf[~inside] == SENTINEL).all())


@pytest.mark.parametrize("T", [65, 130])
def test_quantizer_and_scale_map_bit_for_bit(T):
    """Against a weight that dequantizes to exactly 448 I every output is one exact product, so y is the
    quantizer's value of that element: any wrong byte, block or scale lane shows as a wrong output."""
    K = 512
    q, s = ops.pack_weight_fp8(448.0 * torch.eye(K, device=DEV))
    w8 = ops.w8_from_fp8(q)
    assert torch.equal(ops.unpack_weight_w8(w8, s, torch.float32), 448.0 * torch.eye(K, device=DEV))
    assert bool((s == 1.0).all())
    g = torch.Generator(device=DEV).manual_seed(T)
    x = (torch.randn(T, K, device=DEV, generator=g) * torch.logspace(-2, 2, K, device=DEV)).to(torch.bfloat16)
    x[5, :64] = 0
    x[7] = 0
    y = ops.linear_mx_rows(x, w8, s)
    assert torch.equal(y, (448.0 * ops.mx_block_quant(x.float())).to(torch.bfloat16))


@pytest.mark.parametrize("N,K,epi,T", [(560, 512, 0, 65), (2048, 512, 1, 300)])
def test_strided_input_and_rows_past_t(N, K, epi, T):
    w8, ws, _ = weight(N, K)
    x = rows(T, K, T)
    y = ops.linear_mx_rows(x, w8, ws, epilogue=epi)
    wide = torch.full((T + 20, K + 8), float("nan"), dtype=torch.bfloat16, device=DEV)
    wide[:T, :K] = x
    assert wide[:T, :K].stride(0) == K + 8
    got = ops.linear_mx_rows(wide[:T, :K], w8, ws, epilogue=epi)
    assert torch.equal(got, y) and bool(torch.isfinite(got.float()).all())


def test_uncovered_shapes_and_bad_arguments_launch_nothing():
    assert ops.mx_rows_ok(65, 768, 512, 0) and ops.mx_rows_ok(1 << 20, 48, 128, 0)
    assert not ops.mx_rows_ok(64, 768, 512, 0) and not ops.mx_rows_ok(65, 768, 96, 0)
    assert not ops.mx_rows_ok(65, 48, 512, 1)
    w8, ws, _ = weight(768, 512)
    x = rows(65, 512, 1)
    ax, as_ = ops.mx_rows_buffers(65, 512, DEV)
    out = torch.full((65, 768), SENTINEL, dtype=torch.bfloat16, device=DEV)
    with pytest.raises(RuntimeError, match="x must be bf16"):
        torch.ops.mpamd.quant_mx_rows(x.half(), ax, as_)
    with pytest.raises(RuntimeError, match="ax must be"):
        torch.ops.mpamd.quant_mx_rows(x, ax.view(-1)[:-16], as_)
    with pytest.raises(RuntimeError, match="ax must be"):
        torch.ops.mpamd.gemm_mx_rows(ax.view(-1)[:-16], as_, w8, ws, out, 65, 0)
    with pytest.raises(RuntimeError, match="as must be"):
        torch.ops.mpamd.gemm_mx_rows(ax, as_[:1], w8, ws, out, 65, 0)
    with pytest.raises(RuntimeError, match="out must be"):
        torch.ops.mpamd.gemm_mx_rows(ax, as_, w8, ws, out[:, :384], 65, 0)
    with pytest.raises(ValueError, match="out must be"):
        ops.linear_mx_rows(x, w8, ws, out=out[:64])
    with pytest.raises(RuntimeError, match="no kernel covers"):
        ops.linear_mx_rows(x[:64], w8, ws, out=out[:64])
    torch.cuda.synchronize()
    assert bool((out == SENTINEL).all())


# ------------------------------------------------------------------ executor
MX_ROUTE_FIGURE = 0.1263  # fp32 emulation (docstring below)
MX_ROUTE_BOUND = 2 * MX_ROUTE_FIGURE


def test_mx_stage_takes_the_route_only_when_asked(monkeypatch):
    """A 2-layer Llama-3-8B-shaped fp8 stage in MX mode, an 80 + 9-token prefill.  MPAMD_MX_ROWS=4096 sends all
    four projections of every layer to ops.linear_mx_rows and none to ops.linear_w8_rows; unset or 64 is the
    parent's route, bit for bit.

    Bound on the relative Frobenius distance of the route-on logits to the route-off logits: an fp32 torch
    run on the CPU over the same dequantized weights and prompts, once with ops.mx_block_quant on the four
    projection inputs of every layer and once without, puts the two sets of last-token logits 0.1263 apart
    (0.139 for the 80-token prompt alone, 0.112 for the 9-token one); the bound is twice that, 0.2526 (bf16
    intermediates and summation order, which the emulation does not have)."""
    cfg = dataclasses.replace(resolve_model("llama3-8b"), num_hidden_layers=2)
    calls = {"mx": 0, "w8": 0}

    def counted(key, f):
        def run(*a, **kw):
            calls[key] += 1
            return f(*a, **kw)
        return run

    monkeypatch.setattr(ops, "linear_mx_rows", counted("mx", ops.linear_mx_rows))
    monkeypatch.setattr(ops, "linear_w8_rows", counted("w8", ops.linear_w8_rows))
    monkeypatch.setenv("MPAMD_FP8_MODE", "mx")
    g = torch.Generator().manual_seed(3)
    ids = torch.cat([torch.randint(0, cfg.vocab_size, (n,), generator=g) for n in (80, 9)]).to(DEV)
    logits, seen = {}, {}
    for cap in (None, "4096", "64"):
        monkeypatch.delenv("MPAMD_MX_ROWS", raising=False)
        if cap is not None:
            monkeypatch.setenv("MPAMD_MX_ROWS", cap)
        w = random_stage_weights(cfg, 0, 2, has_embed=True, has_head=True, device=DEV, seed=3, fp8=True)
        ex = StageExecutor(cfg, w, DEV, max_sessions=4, max_seq_len=128, kv_cache_bytes=256 << 20,
                           max_tokens_per_step=128, warmup=False)
        assert ex._mx
        calls.update(mx=0, w8=0)
        logits[cap] = ex.forward([("a", 80), ("b", 9)], ids).float().clone()
        seen[cap] = dict(calls)
        del ex, w
        torch.cuda.empty_cache()
    assert seen["4096"] == {"mx": 4 * cfg.num_hidden_layers, "w8": 0}
    assert seen[None]["mx"] == 0 and seen["64"]["mx"] == 0
    assert torch.equal(logits[None], logits["64"])
    on, off = logits["4096"], logits[None]
    assert bool(torch.isfinite(on).all())
    rel = float((on - off).norm() / off.norm())
    print(f"route on vs off: rel fro {rel:.4g} (bound {MX_ROUTE_BOUND:.4g})")
    assert rel < MX_ROUTE_BOUND
