"""ops.linear_mx_rows on the CPU (the torch form the GPU kernel is tested against), the MPAMD_MX_ROWS switch
and the executor route's first condition: a CPU fp8 stage never takes it."""
import pytest
import torch

from src import ops
from src.models.config import resolve_model
from src.models.weights import random_stage_weights
from src.ops import reference as ref
from src.runtime.executor import MX_ROWS_DEFAULT, StageExecutor


@pytest.mark.parametrize("epilogue", [0, 1])
def test_cpu_form_equals_the_reference_linear_on_the_block_quantized_activation(epilogue):
    g = torch.Generator().manual_seed(epilogue)
    q, s = ops.pack_weight_fp8(0.02 * torch.randn(64, 128, generator=g))
    w8 = ops.w8_from_fp8(q)
    x = torch.randn(65, 128, generator=g).to(torch.bfloat16)
    xq = ops.mx_block_quant(x).to(torch.bfloat16)
    assert torch.equal(xq.float(), ops.mx_block_quant(x)) and not torch.equal(xq, x)
    want = ref.linear(xq, ops.unpack_weight_w8(w8, s, x.dtype), epilogue=epilogue)
    out = torch.empty(65, 32 if epilogue else 64, dtype=torch.bfloat16)
    assert ops.linear_mx_rows(x, w8, s, out=out, epilogue=epilogue) is out
    assert torch.equal(out, want) and torch.equal(ops.linear_mx_rows(x, w8, s, epilogue=epilogue), want)
    with pytest.raises(ValueError, match="out must be"):
        ops.linear_mx_rows(x, w8, s, out=out[:, :16], epilogue=epilogue)


def _cpu_stage(monkeypatch, cap):
    monkeypatch.setenv("MPAMD_FP8_MODE", "mx")
    monkeypatch.delenv("MPAMD_MX_ROWS", raising=False)
    if cap is not None:
        monkeypatch.setenv("MPAMD_MX_ROWS", cap)
    cfg = resolve_model("tiny-llama")
    w = random_stage_weights(cfg, 0, 2, has_embed=True, has_head=True, device="cpu", dtype=torch.float32, seed=1,
                             quant_type="fp8")
    return cfg, StageExecutor(cfg, w, "cpu", kv_cache_bytes=16 << 20, max_sessions=2, max_seq_len=128)


def test_the_switch_is_off_by_default(monkeypatch):
    assert MX_ROWS_DEFAULT == 0
    assert _cpu_stage(monkeypatch, None)[1]._mx_rows_cap == 0
    assert _cpu_stage(monkeypatch, "4096")[1]._mx_rows_cap == 4096


def test_a_cpu_fp8_executor_never_takes_the_route(monkeypatch):
    calls = [0]

    def counted(*a, _f=ops.linear_mx_rows, **kw):
        calls[0] += 1
        return _f(*a, **kw)

    monkeypatch.setattr(ops, "linear_mx_rows", counted)
    cfg, ex = _cpu_stage(monkeypatch, "4096")
    ids = torch.arange(70) % cfg.vocab_size
    assert torch.isfinite(ex.forward([("a", 70)], ids).float()).all()
    assert calls[0] == 0
