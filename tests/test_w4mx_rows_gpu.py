"""The W4A8-MX GEMM above 64 rows (csrc/gemm_w4mx_rows.hip: natural-block quantizer + block-scaled MFMA GEMM on
MXFP4 weights in place) and the executor route onto it, on the GPU.

Shapes and weights are test_w4_rows_gpu.py's (its docstring says what each reaches; (560, 384) is three
k-stages), plus a SwiGLU case with three stages.  The reference multiplies ops.mxn_block_quant(x), the exact
values the quantizer produces, with the dequantized weight in fp64: what is left is fp32 summation order and
one bf16 rounding.
"""
import dataclasses

import pytest
import torch

from src import ops
from src.models.config import resolve_model
from src.models.weights import random_stage_weights
from src.ops import reference as ref
from src.runtime.executor import StageExecutor

from .test_moe_fp8_gpu import rows
from .test_moe_rows_gpu import check
from .test_w4_rows_gpu import DEV, FULL, SENTINEL, SHAPES, TS, oracle, weight

pytestmark = pytest.mark.gpu
CASES = [s + (T,) for s in SHAPES for T in TS] + [(2048, 384, 1, 300)] + FULL


@pytest.mark.parametrize("N,K,epi,T", CASES)
def test_matches_the_fp64_reference_repeats_bit_for_bit_and_stays_inside_out(N, K, epi, T):
    assert ops.w4mx_rows_ok(T, N, K, epi)
    w4, s4, wd = weight(N, K)
    x, nc = rows(T, K, T), N // 2 if epi else N
    buf = torch.full((T + 3, nc + 24), SENTINEL, dtype=torch.bfloat16, device=DEV)
    out = buf[:T, 8:8 + nc]
    assert ops.linear_w4mx_rows(x, w4, s4, out=out, epilogue=epi) is out
    check(out, oracle(ops.mxn_block_quant(x.float()), wd, epi), f"N={N} K={K} epilogue={epi} T={T}")
    assert torch.equal(ops.linear_w4mx_rows(x, w4, s4, epilogue=epi), out)
    inside = torch.zeros_like(buf, dtype=torch.bool)
    inside[:T, 8:8 + nc] = True
    assert bool((buf[~inside] == SENTINEL).all())


@pytest.mark.parametrize("T", [65, 130])
def test_activation_map_bit_for_bit(T):
    """Against a weight that dequantizes to exactly I every output is one exact product, so y is the quantizer's
    value of that element: any wrong byte, block or scale lane shows as a wrong output."""
    K = 512
    w4, s4 = ops.pack_weight_w4(torch.eye(K, device=DEV))
    assert torch.equal(ops.unpack_weight_w4(w4, s4, torch.float32), torch.eye(K, device=DEV))
    g = torch.Generator(device=DEV).manual_seed(T)
    x = (torch.randn(T, K, device=DEV, generator=g) * torch.logspace(-2, 2, K, device=DEV)).to(torch.bfloat16)
    x[5, :64] = 0
    x[7] = 0
    assert torch.equal(ops.linear_w4mx_rows(x, w4, s4), ops.mxn_block_quant(x.float()).to(torch.bfloat16))


@pytest.mark.parametrize("T", [128, 256])
def test_weight_map_bit_for_bit(T):
    """x = I quantizes to itself (256 x 2^-8), so y^T is the dequantized weight: any wrong nibble, lane exchange
    or scale byte is a wrong element.  Magnitudes depend on the column and on the 32-deep k-block."""
    N = K = T
    N += 16
    g = torch.Generator(device=DEV).manual_seed(T)
    mag = torch.exp2(torch.randint(-6, 7, (N, K // 32), device=DEV, generator=g).float()).repeat_interleave(32, 1)
    w4, s4 = ops.pack_weight_w4(0.02 * torch.randn(N, K, device=DEV, generator=g) * mag)
    x = torch.eye(K, dtype=torch.bfloat16, device=DEV)
    assert torch.equal(ops.mxn_block_quant(x), x.float())
    assert torch.equal(ops.linear_w4mx_rows(x, w4, s4).t(), ops.unpack_weight_w4(w4, s4))


@pytest.mark.parametrize("N,K,epi,T", [(560, 384, 0, 65), (2048, 256, 1, 300)])
def test_strided_input_and_rows_past_t(N, K, epi, T):
    w4, s4, _ = weight(N, K)
    x = rows(T, K, T)
    y = ops.linear_w4mx_rows(x, w4, s4, epilogue=epi)
    wide = torch.full((T + 20, K + 8), float("nan"), dtype=torch.bfloat16, device=DEV)
    wide[:T, :K] = x
    assert wide[:T, :K].stride(0) == K + 8
    got = ops.linear_w4mx_rows(wide[:T, :K], w4, s4, epilogue=epi)
    assert torch.equal(got, y) and bool(torch.isfinite(got.float()).all())


def test_uncovered_shapes_and_bad_arguments_launch_nothing():
    assert ops.w4mx_rows_ok(65, 768, 128, 0) and ops.w4mx_rows_ok(1 << 20, 48, 128, 0)
    assert not ops.w4mx_rows_ok(64, 768, 128, 0) and not ops.w4mx_rows_ok(65, 768, 96, 0)
    assert not ops.w4mx_rows_ok(65, 48, 128, 1)
    w4, s4, _ = weight(768, 128)
    x = rows(65, 128, 1)
    axn, asn = ops.mx_rows_buffers(65, 128, DEV)
    out = torch.full((65, 768), SENTINEL, dtype=torch.bfloat16, device=DEV)
    with pytest.raises(RuntimeError, match="x must be bf16"):
        torch.ops.mpamd.quant_mxn_rows(x.half(), axn, asn)
    with pytest.raises(RuntimeError, match="ax must be"):
        torch.ops.mpamd.quant_mxn_rows(x, axn.view(-1)[:-16], asn)
    with pytest.raises(RuntimeError, match="ax must be"):
        torch.ops.mpamd.gemm_w4mx_rows(axn.view(-1)[:-16], asn, w4, s4, out, 65, 0)
    with pytest.raises(RuntimeError, match="as must be"):
        torch.ops.mpamd.gemm_w4mx_rows(axn, asn.view(-1)[:-4], w4, s4, out, 65, 0)
    with pytest.raises(RuntimeError, match="s4 must be"):
        torch.ops.mpamd.gemm_w4mx_rows(axn, asn, w4, s4[:-1], out, 65, 0)
    with pytest.raises(RuntimeError, match="out must be"):
        torch.ops.mpamd.gemm_w4mx_rows(axn, asn, w4, s4, out[:, :384], 65, 0)
    with pytest.raises(ValueError, match="out must be"):
        ops.linear_w4mx_rows(x, w4, s4, out=out[:64])
    with pytest.raises(RuntimeError, match="no kernel covers"):
        ops.linear_w4mx_rows(x[:64], w4, s4, out=out[:64])
    torch.cuda.synchronize()
    assert bool((out == SENTINEL).all())


# ------------------------------------------------------------------ executor
W4MX_ROUTE_FIGURE = 0.0582  # fp32 emulation (docstring below)
W4MX_ROUTE_BOUND = 2 * W4MX_ROUTE_FIGURE


def two_layer_stage(device):
    """(cfg, MXFP4 weights, fp32 weights whose projections are the dequantized MXFP4 ones) of a 2-layer
    small-llama stage."""
    cfg = dataclasses.replace(resolve_model("small-llama"), num_hidden_layers=2)
    w = random_stage_weights(cfg, 0, 2, has_embed=True, has_head=True, device=device, seed=5)
    wd = random_stage_weights(cfg, 0, 2, has_embed=True, has_head=True, device=device, seed=5, dtype=torch.float32)
    w.quantize_mxfp4(drop_dense=True)
    for L, Ld in zip(w.layers, wd.layers):
        for name in L.PROJ:
            setattr(Ld, name, ref.unpack_weight_w4(getattr(L, name + "_w4"), getattr(L, name + "_s4"), torch.float32))
    return cfg, w, wd


def test_mxfp4_stage_takes_the_route_only_when_asked(monkeypatch):
    """A 2-layer small-llama MXFP4 stage, an 80 + 9-token prefill.  MPAMD_W4_MX_ROWS=4096 sends all four
    projections of every layer to ops.linear_w4mx_rows and none to ops.linear_w4_rows (which MPAMD_W4_ROWS=4096
    would otherwise take); unset or 64 is the parent's route, bit for bit.

    Bound on the relative Frobenius distance of the route-on logits to the route-off logits: an fp32 torch run
    over the same dequantized weights and prompts, once with ops.mxn_block_quant on the four projection inputs
    of every layer and once without, puts the two sets of last-token logits 0.0582 apart (0.0647 for the
    80-token prompt alone, 0.0509 for the 9-token one; 0.0540 with weights drawn by the CPU generator); the bound
    is twice that, 0.1164 (bf16 intermediates and summation order, which the emulation does not have)."""
    calls = {"w4mx": 0, "w4": 0}

    def counted(key, f):
        def run(*a, **kw):
            calls[key] += 1
            return f(*a, **kw)
        return run

    monkeypatch.setattr(ops, "linear_w4mx_rows", counted("w4mx", ops.linear_w4mx_rows))
    monkeypatch.setattr(ops, "linear_w4_rows", counted("w4", ops.linear_w4_rows))
    monkeypatch.setenv("MPAMD_W4_ROWS", "4096")
    cfg, w, _ = two_layer_stage(DEV)
    g = torch.Generator().manual_seed(3)
    ids = torch.cat([torch.randint(0, cfg.vocab_size, (n,), generator=g) for n in (80, 9)]).to(DEV)
    logits, seen = {}, {}
    for cap in (None, "4096", "64"):
        monkeypatch.delenv("MPAMD_W4_MX_ROWS", raising=False)
        if cap is not None:
            monkeypatch.setenv("MPAMD_W4_MX_ROWS", cap)
        ex = StageExecutor(cfg, w, DEV, kv_cache_bytes=128 << 20, max_sessions=4, max_seq_len=128, use_graphs=False)
        assert ex._w4
        calls.update(w4mx=0, w4=0)
        logits[cap] = ex.forward([("a", 80), ("b", 9)], ids).float().clone()
        seen[cap] = dict(calls)
        del ex
    per_step = 4 * cfg.num_hidden_layers
    assert seen["4096"] == {"w4mx": per_step, "w4": 0}
    assert seen[None] == {"w4mx": 0, "w4": per_step} and seen["64"] == seen[None]
    assert torch.equal(logits[None], logits["64"])
    on, off = logits["4096"], logits[None]
    assert bool(torch.isfinite(on).all())
    rel = float((on - off).norm() / off.norm())
    print(f"route on vs off: rel fro {rel:.4g} (bound {W4MX_ROUTE_BOUND:.4g})")
    assert rel < W4MX_ROUTE_BOUND
