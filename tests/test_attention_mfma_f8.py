"""The fp8-cache forms of the MFMA GQA decode ops off the GPU: ``ops.attention_mfma_f8`` /
``ops.attention_mfma_rope_f8`` fall back to the reference forms on a ``KVF8``, refuse bf16 caches,
the three bf16 MFMA / FA2 ops keep refusing a ``KVF8``, and the executor's ``gqa_decode_mfma_f8``
attribute follows the model's group size and the ``MPAMD_KV_FP8_MFMA`` switch."""
import dataclasses

import pytest
import torch

from src import ops
from src.models.config import resolve_model
from src.models.reference_model import reference_forward
from src.models.weights import random_stage_weights
from src.runtime.executor import StageExecutor


def _case(T=5, nh=8, nkv=2, D=64, ps=64):
    g = torch.Generator().manual_seed(3)
    qkv = torch.randn(T, (nh + 2 * nkv) * D, generator=g).to(torch.bfloat16)
    dense = torch.randn(2, 2, nkv, ps, D, generator=g).to(torch.bfloat16)
    bt = torch.tensor([[1, 0]], dtype=torch.int32)
    q_seq, q_ctx = torch.zeros(T, dtype=torch.int32), torch.arange(1, T + 1, dtype=torch.int32)
    pos = torch.arange(T)
    slots = torch.tensor([ps + 0, ps + 1, ps + 2, -1, ps + 4])
    cos, sin = ops.rope_cos_sin(D, 64, 10000.0, "cpu")
    fresh = lambda: (ops.KVF8.from_dense(dense[0]), ops.KVF8.from_dense(dense[1]))  # noqa: E731
    return dict(nh=nh, nkv=nkv, D=D, qkv=qkv, dense=dense, bt=bt, q_seq=q_seq, q_ctx=q_ctx, pos=pos, slots=slots,
                cos=cos, sin=sin, fresh=fresh)


def _same_cache(a, b):
    return torch.equal(a.codes, b.codes) and torch.equal(a.scales, b.scales)


def test_cpu_attention_mfma_f8_is_paged_attention_on_the_fp8_cache():
    c = _case()
    kf, vf = c["fresh"]()
    got = ops.attention_mfma_f8(c["qkv"], kf, vf, c["bt"], c["q_seq"], c["q_ctx"], None, c["nh"], c["nkv"], 0.125)
    want = ops.paged_attention(c["qkv"], kf, vf, c["bt"], c["q_seq"], c["q_ctx"], c["nh"], c["nkv"], 0.125)
    assert torch.equal(got, want) and bool(got.float().abs().sum() > 0)
    gp = ops.attention_mfma_f8(c["qkv"], kf, vf, c["bt"], c["q_seq"], c["q_ctx"], None, c["nh"], c["nkv"], 0.125,
                               packed=True)
    assert torch.equal(ops.unpack_act(gp, 5, c["nh"] * c["D"]), want)


@pytest.mark.parametrize("fold", [False, True])
def test_cpu_attention_mfma_rope_f8_is_paged_attention_rope_on_the_fp8_cache(fold):
    c = _case()
    qkv, part = c["qkv"], None
    if fold:  # two slabs that sum to other rows than ``qkv``: the op must read the slabs
        g = torch.Generator().manual_seed(9)
        slabs = torch.randn(2, *qkv.shape, generator=g)
        part = (slabs, None, 1.0 / 64, 1e-5)
        assert not torch.equal(ops.reduce_qkv_part(part), qkv)
    args = (c["bt"], c["q_seq"], c["q_ctx"])
    rope = (c["pos"], c["cos"], c["sin"], c["slots"], c["nh"], c["nkv"], 0.125)
    k1, v1 = c["fresh"]()
    q_in = qkv.clone()
    got = ops.attention_mfma_rope_f8(qkv, k1, v1, *args, None, *rope, qkv_part=part)
    assert torch.equal(qkv, q_in), "the fused op must not modify qkv"
    k2, v2 = c["fresh"]()
    want = ops.paged_attention_rope(qkv, k2, v2, *args, *rope, qkv_part=part)
    assert torch.equal(got, want)
    assert _same_cache(k1, k2) and _same_cache(v1, v2)
    k0, v0 = c["fresh"]()
    assert not _same_cache(k1, k0) and not _same_cache(v1, v0)  # the new tokens were written
    if fold:  # ... and equal the same step on the reduced rows
        k3, v3 = c["fresh"]()
        o3 = ops.attention_mfma_rope_f8(ops.reduce_qkv_part(part), k3, v3, *args, None, *rope)
        assert torch.equal(o3, got) and _same_cache(k3, k1) and _same_cache(v3, v1)


def test_cpu_f8_ops_refuse_bf16_caches_and_the_bf16_ops_refuse_fp8_caches():
    c = _case()
    kf, vf = c["fresh"]()
    kb, vb = kf.dequant(), vf.dequant()
    args = (c["bt"], c["q_seq"], c["q_ctx"], None)
    rope = (c["pos"], c["cos"], c["sin"], c["slots"], c["nh"], c["nkv"], 1.0)
    with pytest.raises(TypeError):
        ops.attention_mfma_f8(c["qkv"], kb, vb, *args, c["nh"], c["nkv"], 1.0)
    with pytest.raises(TypeError):
        ops.attention_mfma_f8(c["qkv"], kf, vb, *args, c["nh"], c["nkv"], 1.0)
    with pytest.raises(TypeError):
        ops.attention_mfma_rope_f8(c["qkv"], kb, vb, *args, *rope)
    for call in (lambda: ops.attention_mfma(c["qkv"], kf, vf, *args, c["nh"], c["nkv"], 1.0),
                 lambda: ops.attention_fa(c["qkv"], kf, vf, *args, c["nh"], c["nkv"], 1.0),
                 lambda: ops.attention_mfma_rope(c["qkv"], kf, vf, *args, *rope)):
        with pytest.raises(NotImplementedError, match="fp8 KV"):
            call()


# ------------------------------------------------------------------------------------------ executor
def _gqa4():
    return dataclasses.replace(resolve_model("small-llama"), num_key_value_heads=1, name="small-llama-gqa4")


def _cpu_executor(cfg, **kw):
    w = random_stage_weights(cfg, 0, cfg.num_hidden_layers, has_embed=True, has_head=True, device="cpu",
                             dtype=torch.float32, seed=7)
    return w, StageExecutor(cfg, w, "cpu", dtype=torch.float32, kv_cache_bytes=32 << 20, max_sessions=8,
                            max_seq_len=256, **kw)


@pytest.mark.parametrize("env,want", [(None, True), ("1", True), ("0", False)])
def test_cpu_executor_gqa_decode_mfma_f8_follows_the_switch(env, want, monkeypatch):
    if env is None:
        monkeypatch.delenv("MPAMD_KV_FP8_MFMA", raising=False)
    else:
        monkeypatch.setenv("MPAMD_KV_FP8_MFMA", env)
    cfg = _gqa4()
    assert cfg.num_attention_heads // cfg.num_key_value_heads == 4 and cfg.head_dim == 128
    w, ex = _cpu_executor(cfg, kv_cache_dtype="fp8")
    assert bool(ex.gqa_decode_mfma_f8) is want and not ex.gqa_decode_mfma
    assert ex._attn_min_part == (256 if want else 64)
    # a decode step still tracks the fake-quantized oracle
    g = torch.Generator().manual_seed(0)
    seqs = [torch.randint(0, cfg.vocab_size, (n,), generator=g) for n in (13, 70)]  # one crosses a page
    names = ["a", "b"]
    lg = ex.forward([(n, len(s)) for n, s in zip(names, seqs)], torch.cat(seqs))
    nxt = torch.argmax(lg, -1)
    seqs = [torch.cat([s, nxt[i:i + 1]]) for i, s in enumerate(seqs)]
    lg = ex.forward([(n, 1) for n in names], nxt)
    hook = lambda k, v: (ops.fake_quant_kv_fp8(k), ops.fake_quant_kv_fp8(v))  # noqa: E731
    for i, s in enumerate(seqs):
        ref_lg = reference_forward([w], s, kv_hook=hook)[-1]
        cos = torch.nn.functional.cosine_similarity(lg[i].float(), ref_lg, dim=0)
        assert float(cos) > 0.99, (i, float(cos))


def test_cpu_executor_gqa_decode_mfma_f8_off_for_bf16_small_groups_and_mha(monkeypatch):
    monkeypatch.delenv("MPAMD_KV_FP8_MFMA", raising=False)
    _, ex = _cpu_executor(_gqa4())  # the default bf16 cache keeps the bf16 kernel
    assert ex.gqa_decode_mfma and not ex.gqa_decode_mfma_f8
    for model in ("tiny-llama", "small-llama"):  # nrep 2, MHA
        _, ex = _cpu_executor(resolve_model(model), kv_cache_dtype="fp8")
        assert not ex.gqa_decode_mfma_f8 and not ex.gqa_decode_mfma
