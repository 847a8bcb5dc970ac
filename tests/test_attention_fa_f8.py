"""The fp8-cache form of the FA2 prefill op off the GPU: ``ops.attention_fa_f8`` falls back to the
reference form on a ``KVF8``, refuses bf16 and mixed caches, ``ops.attention_fa`` keeps refusing a
``KVF8``, and the executor's ``prefill_fa_f8`` attribute follows ``ops.fa_ok`` of the model and the
``MPAMD_KV_FP8_FA`` switch."""
import pytest
import torch

from src import ops
from src.models.config import resolve_model
from src.models.reference_model import reference_forward
from src.models.weights import random_stage_weights
from src.runtime.executor import StageExecutor


def _case(T=70, nh=8, nkv=2, D=128, ps=64):
    """One prompt of T tokens over two pages (causal: ctx = i + 1)."""
    g = torch.Generator().manual_seed(3)
    qkv = torch.randn(T, (nh + 2 * nkv) * D, generator=g).to(torch.bfloat16)
    dense = torch.randn(2, 3, nkv, ps, D, generator=g).to(torch.bfloat16)
    bt = torch.tensor([[2, 0]], dtype=torch.int32)
    q_seq, q_ctx = torch.zeros(T, dtype=torch.int32), torch.arange(1, T + 1, dtype=torch.int32)
    fb = torch.from_numpy(ops.fa_blocks([T], nh // nkv, 4))
    return dict(nh=nh, nkv=nkv, D=D, qkv=qkv, kf=ops.KVF8.from_dense(dense[0]), vf=ops.KVF8.from_dense(dense[1]),
                args=(bt, q_seq, q_ctx, fb))


def test_cpu_attention_fa_f8_is_paged_attention_on_the_fp8_cache():
    c = _case()
    got = ops.attention_fa_f8(c["qkv"], c["kf"], c["vf"], *c["args"], c["nh"], c["nkv"], 0.125)
    want = ops.paged_attention(c["qkv"], c["kf"], c["vf"], *c["args"][:3], c["nh"], c["nkv"], 0.125)
    assert torch.equal(got, want) and bool(got.float().abs().sum() > 0)
    out = torch.empty_like(want)
    assert ops.attention_fa_f8(c["qkv"], c["kf"], c["vf"], *c["args"], c["nh"], c["nkv"], 0.125, out=out, waves=8,
                               num_parts=2, pair=False) is out
    assert torch.equal(out, want)


def test_cpu_attention_fa_f8_refuses_bf16_caches_and_attention_fa_refuses_fp8_caches():
    c = _case(T=5)
    kf, vf = c["kf"], c["vf"]
    kb, vb = kf.dequant(), vf.dequant()
    for k, v in ((kb, vb), (kf, vb), (kb, vf)):
        with pytest.raises(TypeError):
            ops.attention_fa_f8(c["qkv"], k, v, *c["args"], c["nh"], c["nkv"], 1.0)
    for k, v in ((kf, vf), (kf, vb), (kb, vf)):
        with pytest.raises(NotImplementedError, match="fp8 KV"):
            ops.attention_fa(c["qkv"], k, v, *c["args"], c["nh"], c["nkv"], 1.0)


def _cpu_executor(cfg, **kw):
    w = random_stage_weights(cfg, 0, cfg.num_hidden_layers, has_embed=True, has_head=True, device="cpu",
                             dtype=torch.float32, seed=7)
    return w, StageExecutor(cfg, w, "cpu", dtype=torch.float32, kv_cache_bytes=32 << 20, max_sessions=8,
                            max_seq_len=256, **kw)


@pytest.mark.parametrize("model", ["small-llama", "tiny-llama"])
def test_cpu_executor_prefill_fa_f8_follows_fa_ok(model, monkeypatch):
    monkeypatch.delenv("MPAMD_KV_FP8_FA", raising=False)
    cfg = resolve_model(model)
    ok = ops.fa_ok(cfg.num_attention_heads, cfg.num_key_value_heads, cfg.head_dim, 64)
    assert ok is (model == "small-llama")
    _, ex = _cpu_executor(cfg, kv_cache_dtype="fp8")
    assert ex.cache.is_fp8 and bool(ex.prefill_fa_f8) is ok
    _, ex = _cpu_executor(cfg)  # a bf16 cache never takes the fp8 form
    assert not ex.prefill_fa_f8


@pytest.mark.parametrize("env,want", [(None, True), ("1", True), ("0", False)])
def test_cpu_executor_prefill_fa_f8_follows_the_switch(env, want, monkeypatch):
    if env is None:
        monkeypatch.delenv("MPAMD_KV_FP8_FA", raising=False)
    else:
        monkeypatch.setenv("MPAMD_KV_FP8_FA", env)
    cfg = resolve_model("small-llama")
    w, ex = _cpu_executor(cfg, kv_cache_dtype="fp8")
    assert bool(ex.prefill_fa_f8) is want
    # a prefill step still tracks the fake-quantized oracle
    g = torch.Generator().manual_seed(0)
    seqs = [torch.randint(0, cfg.vocab_size, (n,), generator=g) for n in (13, 70)]  # one crosses a page
    lg = ex.forward([(n, len(s)) for n, s in zip("ab", seqs)], torch.cat(seqs))
    hook = lambda k, v: (ops.fake_quant_kv_fp8(k), ops.fake_quant_kv_fp8(v))  # noqa: E731
    for i, s in enumerate(seqs):
        ref_lg = reference_forward([w], s, kv_hook=hook)[-1]
        cos = torch.nn.functional.cosine_similarity(lg[i].float(), ref_lg, dim=0)
        assert float(cos) > 0.99, (i, float(cos))
