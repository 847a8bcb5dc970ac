"""ops.mxn_block_quant and ops.linear_w4mx_rows on the CPU (the torch forms the GPU kernels are tested against),
the MPAMD_W4_MX_ROWS switch and the executor route's first condition: a CPU MXFP4 stage never takes it."""
import pytest
import torch

from src import ops
from src.models.config import resolve_model
from src.models.weights import random_stage_weights
from src.ops import reference as ref
from src.runtime.executor import W4_MX_ROWS_DEFAULT, StageExecutor


def test_natural_blocks_are_32_consecutive_k():
    """An element of 2^20 drives the N(0, 1) values of its block below e4m3's smallest subnormal: exactly its
    own 32 consecutive k change (mx_block_quant's blocks are not contiguous), and every block is within e4m3's
    half ulp (2^-4 relative) of its input."""
    g = torch.Generator().manual_seed(0)
    x = torch.randn(3, 256, generator=g).to(torch.bfloat16).float()
    y = x.clone()
    y[1, 70] = 2.0 ** 20
    d = (ops.mxn_block_quant(y) != ops.mxn_block_quant(x)).nonzero()
    assert bool((d[:, 0] == 1).all()) and d[:, 1].tolist() == list(range(64, 96))
    assert float((ops.mxn_block_quant(x) - x).abs().max()) <= 2.0 ** -4 * float(x.abs().max())
    assert not torch.equal(ops.mxn_block_quant(y), ops.mx_block_quant(y))


@pytest.mark.parametrize("epilogue", [0, 1])
def test_cpu_form_equals_the_reference_linear_on_the_block_quantized_activation(epilogue):
    g = torch.Generator().manual_seed(epilogue)
    w4, s4 = ops.pack_weight_w4(0.02 * torch.randn(64, 128, generator=g))
    x = torch.randn(65, 128, generator=g).to(torch.bfloat16)
    xq = ops.mxn_block_quant(x).to(torch.bfloat16)
    assert torch.equal(xq.float(), ops.mxn_block_quant(x)) and not torch.equal(xq, x)
    want = ref.linear(xq, ops.unpack_weight_w4(w4, s4, x.dtype), epilogue=epilogue)
    out = torch.empty(65, 32 if epilogue else 64, dtype=torch.bfloat16)
    assert ops.linear_w4mx_rows(x, w4, s4, out=out, epilogue=epilogue) is out
    assert torch.equal(out, want) and torch.equal(ops.linear_w4mx_rows(x, w4, s4, epilogue=epilogue), want)
    with pytest.raises(ValueError, match="out must be"):
        ops.linear_w4mx_rows(x, w4, s4, out=out[:, :16], epilogue=epilogue)


def test_the_switch_is_off_by_default_and_a_cpu_stage_never_takes_the_route(monkeypatch):
    calls = [0]

    def counted(*a, _f=ops.linear_w4mx_rows, **kw):
        calls[0] += 1
        return _f(*a, **kw)

    monkeypatch.setattr(ops, "linear_w4mx_rows", counted)
    cfg = resolve_model("tiny-llama")
    w = random_stage_weights(cfg, 0, 2, has_embed=True, has_head=True, device="cpu", dtype=torch.float32, seed=1,
                             quant_type="mxfp4")
    assert W4_MX_ROWS_DEFAULT == 0
    for cap in (None, "4096"):
        monkeypatch.delenv("MPAMD_W4_MX_ROWS", raising=False)
        if cap is not None:
            monkeypatch.setenv("MPAMD_W4_MX_ROWS", cap)
        ex = StageExecutor(cfg, w, "cpu", kv_cache_bytes=16 << 20, max_sessions=2, max_seq_len=128)
        assert ex._w4_mx_rows_cap == int(cap or 0)
    ids = torch.arange(70) % cfg.vocab_size
    assert torch.isfinite(ex.forward([("a", 70)], ids).float()).all()
    assert calls[0] == 0
