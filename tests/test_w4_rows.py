"""ops.linear_w4_rows on the CPU (the torch form the GPU kernel is tested against) and the executor
route's first condition: a CPU MXFP4 stage never takes it."""
import pytest
import torch

from src import ops
from src.models.config import resolve_model
from src.models.weights import random_stage_weights
from src.ops import reference as ref
from src.runtime.executor import StageExecutor


@pytest.mark.parametrize("epilogue", [0, 1])
def test_cpu_form_equals_the_reference_linear_on_the_dequantized_weight(epilogue):
    g = torch.Generator().manual_seed(epilogue)
    w4, s4 = ops.pack_weight_w4(0.02 * torch.randn(96, 256, generator=g))
    x = torch.randn(70, 256, generator=g).to(torch.bfloat16)
    want = ref.linear(x, ref.unpack_weight_w4(w4, s4, x.dtype), epilogue=epilogue)
    out = torch.empty(70, 48 if epilogue else 96, dtype=torch.bfloat16)
    assert ops.linear_w4_rows(x, w4, s4, out=out, epilogue=epilogue) is out
    assert torch.equal(out, want) and torch.equal(ops.linear_w4_rows(x, w4, s4, epilogue=epilogue), want)
    assert not ops.w4_rows_ok(64, 96, 256, epilogue)
    with pytest.raises(ValueError, match="out must be"):
        ops.linear_w4_rows(x, w4, s4, out=out[:, :32], epilogue=epilogue)


def test_a_cpu_mxfp4_executor_never_takes_the_route(monkeypatch):
    monkeypatch.setenv("MPAMD_W4_ROWS", "4096")
    cfg = resolve_model("tiny-llama")
    w = random_stage_weights(cfg, 0, 2, has_embed=True, has_head=True, device="cpu", dtype=torch.float32, seed=1,
                             quant_type="mxfp4")
    calls = [0]

    def counted(*a, _f=ops.linear_w4_rows, **kw):
        calls[0] += 1
        return _f(*a, **kw)

    monkeypatch.setattr(ops, "linear_w4_rows", counted)
    ex = StageExecutor(cfg, w, "cpu", kv_cache_bytes=16 << 20, max_sessions=2, max_seq_len=128)
    ids = torch.arange(70) % cfg.vocab_size
    assert torch.isfinite(ex.forward([("a", 70)], ids).float()).all()
    assert calls[0] == 0
