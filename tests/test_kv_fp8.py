"""fp8 KV cache off the GPU: the row rule (ops.quant_kv_fp8 / dequant_kv_fp8), the paged cache's fp8
storage, session export / import, the CPU executor against the fake-quantized oracle, and the
``--kv_cache_dtype`` switch up to ``rpc_info``."""
import pytest
import torch

from src import ops
from src.block_utils import auto_num_blocks, kv_cache_bytes_per_block
from src.main import _executor_kwargs, build_parser
from src.models.config import resolve_model
from src.models.reference_model import reference_forward
from src.models.weights import random_stage_weights
from src.runtime.executor import StageExecutor
from src.runtime.kv_cache import PagedKVCache
from src.runtime.kv_layout import export_session_kv, import_session_kv
from src.runtime.session import SessionManager


def _rows(n=64, D=128, seed=0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(n, D, generator=g).to(torch.bfloat16)


def test_dequantized_values_are_exact_in_bf16():
    x = _rows()
    q, e = ops.quant_kv_fp8(x)
    assert q.dtype == torch.uint8 and e.dtype == torch.uint8 and q.shape == x.shape and e.shape == x.shape[:-1]
    f = ops.dequant_kv_fp8(q, e, torch.float32)
    assert torch.equal(f.to(torch.bfloat16).float(), f)
    assert torch.equal(ops.dequant_kv_fp8(q, e).float(), f)


def test_zero_row_gives_unit_scale_and_zero_codes():
    x = _rows(4)
    x[2] = 0
    q, e = ops.quant_kv_fp8(x)
    assert int(e[2]) == 127 and int(q[2].sum()) == 0
    assert torch.count_nonzero(ops.dequant_kv_fp8(q, e)[2]) == 0


def test_largest_code_of_a_row_uses_the_top_octave():
    """amax / scale lies in (224, 448] by the rule (the smallest power-of-two scale that fits 448).
    e4m3 has steps of 32 there, so a scaled amax in (224, 240) rounds DOWN to the code 224: the
    largest |code| lies in [224, 448], and in (224, 448] whenever amax / scale is an e4m3 value."""
    x = torch.cat([_rows(256), _rows(16) * 300, _rows(16) * 1e-3])
    q, e = ops.quant_kv_fp8(x)
    scaled = x.float().abs().amax(-1) * torch.exp2(127.0 - e.float())
    assert bool((scaled > 224).all()) and bool((scaled <= 448).all())
    top = q.view(torch.float8_e4m3fn).float().abs().amax(-1)
    assert bool((top >= 224).all()) and bool((top <= 448).all())
    exact = scaled.to(torch.float8_e4m3fn).float() == scaled  # amax itself representable: no rounding
    assert bool(exact.any()) and torch.equal(top[exact], scaled[exact]) and bool((top[exact] > 224).all())


@pytest.mark.parametrize("mul", [1.0, 300.0, 1e-3])
def test_row_error_is_scale_free(mul):
    x = (_rows(32).float() * mul).to(torch.bfloat16)
    d = ops.fake_quant_kv_fp8(x).float()
    rel = (d - x.float()).norm(dim=-1) / x.float().norm(dim=-1)
    assert float(rel.max()) <= 2.0 ** -4, float(rel.max())


def test_value_round_trip():
    x = torch.cat([_rows(64), _rows(8) * 300, _rows(8) * 1e-3])
    once = ops.fake_quant_kv_fp8(x)
    assert torch.equal(ops.fake_quant_kv_fp8(once), once)


def test_exponent_rule_matches_its_definition():
    """e is the smallest exponent with amax / 2^(e - 127) <= 448 - also at exact powers of two."""
    amax = torch.tensor([448.0, 449.0, 224.0, 1.75, 3.5, 1.0, 2.0 ** -20, 7.0 * 2.0 ** 10, 0.0])
    e = ops.reference.kv_fp8_exponent(amax).float()
    s = torch.exp2(e - 127)
    nz = amax > 0
    assert bool((amax[nz] / s[nz] <= 448).all()) and bool((amax[nz] / (s[nz] / 2) > 448).all())
    assert int(e[-1]) == 127


# --------------------------------------------------------------------------------------- the cache
def test_paged_cache_fp8_storage():
    L, P, nkv, D, ps = 3, 5, 2, 64, 64
    c = PagedKVCache(L, P, nkv, D, ps, torch.bfloat16, "cpu", kv_dtype="fp8")
    assert c.is_fp8 and c.kv_dtype == "fp8"
    for t in (c.k, c.v):
        assert t.shape == (L, P, nkv, ps, D) and t.dtype == torch.uint8
    for t in (c.k_scale, c.v_scale):
        assert t.shape == (L, P, nkv, ps) and t.dtype == torch.uint8
    assert c.bytes_per_page == 2 * L * nkv * ps * (D + 1)
    assert c.nbytes == c.bytes_per_page * P
    assert c.nbytes == sum(t.numel() for t in (c.k, c.v, c.k_scale, c.v_scale))
    kc, vc = c.layer(1)
    assert isinstance(kc, ops.KVF8) and kc.codes.data_ptr() == c.k[1].data_ptr() and \
        vc.scales.data_ptr() == c.v_scale[1].data_ptr() and kc.shape == (P, nkv, ps, D)
    assert torch.count_nonzero(kc.dequant()) == 0  # a fresh cache reads as zeros
    budget = 10 * c.bytes_per_page + 17
    assert PagedKVCache.pages_for_bytes(budget, L, nkv, D, ps, kv_dtype="fp8") == budget // c.bytes_per_page == 10
    bf = PagedKVCache(L, P, nkv, D, ps, torch.bfloat16, "cpu")
    assert not bf.is_fp8 and bf.bytes_per_page == 2 * L * nkv * ps * D * 2 and bf.k.dtype == torch.bfloat16
    assert PagedKVCache.pages_for_bytes(budget, L, nkv, D, ps) == budget // bf.bytes_per_page
    with pytest.raises(ValueError):
        PagedKVCache(L, P, nkv, D, ps, torch.bfloat16, "cpu", kv_dtype="int4")


def test_copy_pages_moves_codes_and_scales():
    c = PagedKVCache(2, 6, 2, 64, 64, torch.bfloat16, "cpu", kv_dtype="fp8")
    g = torch.Generator().manual_seed(1)
    for t in (c.k, c.v, c.k_scale, c.v_scale):
        t.copy_(torch.randint(0, 255, t.shape, generator=g, dtype=torch.uint8))
    before = [t.clone() for t in (c.k, c.v, c.k_scale, c.v_scale)]
    c.copy_pages([1, 4], [0, 5])
    for t, b in zip((c.k, c.v, c.k_scale, c.v_scale), before):
        assert torch.equal(t[:, 0], b[:, 1]) and torch.equal(t[:, 5], b[:, 4])
        assert torch.equal(t[:, 1:5], b[:, 1:5])


def test_export_import_round_trip_on_values():
    L, nkv, D, ps, t = 2, 2, 64, 64, 70  # crosses a page
    c = PagedKVCache(L, 8, nkv, D, ps, torch.bfloat16, "cpu", kv_dtype="fp8")
    sm = SessionManager(c, 4, 256)
    g = torch.Generator().manual_seed(2)
    kv = [(torch.randn(1, nkv, t, D, generator=g).to(torch.bfloat16),
           torch.randn(1, nkv, t, D, generator=g).to(torch.bfloat16) * 5) for _ in range(L)]
    s = import_session_kv(sm, "a", kv)
    out = export_session_kv(c, s)
    for (k, v), (k2, v2) in zip(kv, out):
        assert k2.dtype == torch.bfloat16 and k2.shape == k.shape
        assert torch.equal(k2, ops.fake_quant_kv_fp8(k)) and torch.equal(v2, ops.fake_quant_kv_fp8(v))
    s2 = import_session_kv(sm, "b", out)  # the values survive a second hop (the codes need not)
    for (k2, v2), (k3, v3) in zip(out, export_session_kv(c, s2)):
        assert torch.equal(k2, k3) and torch.equal(v2, v3)


# ------------------------------------------------------------------------------------ op layer (CPU)
def test_cpu_ops_quantize_on_write_and_dequantize_on_read():
    nh, nkv, D, ps, T = 4, 2, 64, 64, 5
    g = torch.Generator().manual_seed(3)
    qkv = torch.randn(T, (nh + 2 * nkv) * D, generator=g).to(torch.bfloat16)
    pos = torch.arange(T)
    slots = torch.tensor([0, 1, 2, -1, 4])
    cos, sin = ops.rope_cos_sin(D, 64, 10000.0, "cpu")
    kb, vb = (torch.zeros(2, nkv, ps, D, dtype=torch.bfloat16) for _ in range(2))
    q1 = qkv.clone()
    ops.rope_kv_write(q1, pos, cos, sin, kb, vb, slots, nh, nkv)
    kf, vf = ops.KVF8.empty(2, nkv, ps, D), ops.KVF8.empty(2, nkv, ps, D)
    q2 = qkv.clone()
    ops.rope_kv_write(q2, pos, cos, sin, kf, vf, slots, nh, nkv)
    assert torch.equal(q1, q2)
    assert torch.equal(kf.dequant(), ops.fake_quant_kv_fp8(kb)) and torch.equal(vf.dequant(), ops.fake_quant_kv_fp8(vb))
    assert int(kf.scales[0, 0, 3]) == 127 and int(kf.codes[0, :, 3].sum()) == 0  # slot -1 wrote nothing
    bt = torch.tensor([[0, 1]], dtype=torch.int32)
    q_seq, q_ctx = torch.zeros(T, dtype=torch.int32), torch.arange(1, T + 1, dtype=torch.int32)
    got = ops.paged_attention(q2, kf, vf, bt, q_seq, q_ctx, nh, nkv, 0.125)
    want = ops.paged_attention(q2, kf.dequant(), vf.dequant(), bt, q_seq, q_ctx, nh, nkv, 0.125)
    assert torch.equal(got, want)
    for name, call in (("attention_mfma", lambda: ops.attention_mfma(q2, kf, vf, bt, q_seq, q_ctx, None, nh, nkv, 1.0)),
                       ("attention_fa", lambda: ops.attention_fa(q2, kf, vf, bt, q_seq, q_ctx, None, nh, nkv, 1.0)),
                       ("attention_mfma_rope", lambda: ops.attention_mfma_rope(
                           qkv, kf, vf, bt, q_seq, q_ctx, None, pos, cos, sin, slots, nh, nkv, 1.0))):
        with pytest.raises(NotImplementedError, match="fp8 KV"):
            call()
    with pytest.raises(TypeError):
        ops.paged_attention(q2, kf, vb, bt, q_seq, q_ctx, nh, nkv, 0.125)


# ------------------------------------------------------------------------------------------ executor
def _fake_quant_hook(k, v):
    return ops.fake_quant_kv_fp8(k), ops.fake_quant_kv_fp8(v)


def test_cpu_executor_fp8_kv_tracks_the_fake_quantized_oracle():
    cfg = resolve_model("tiny-llama")
    w = random_stage_weights(cfg, 0, cfg.num_hidden_layers, has_embed=True, has_head=True, device="cpu",
                             dtype=torch.float32, seed=7)
    ex = StageExecutor(cfg, w, "cpu", dtype=torch.float32, kv_cache_bytes=32 << 20, max_sessions=8, max_seq_len=256,
                       kv_cache_dtype="fp8")
    assert ex.kv_cache_dtype == "fp8" and ex.cache.is_fp8 and ex.cache.k.dtype == torch.uint8
    assert not ex.gqa_decode_mfma
    g = torch.Generator().manual_seed(0)
    seqs = [torch.randint(0, cfg.vocab_size, (n,), generator=g) for n in (13, 70, 1)]  # ragged; one crosses a page
    names = ["a", "b", "c"]
    lg = ex.forward([(n, len(s)) for n, s in zip(names, seqs)], torch.cat(seqs))
    for step in range(4):
        for i, s in enumerate(seqs):
            want = reference_forward([w], s, kv_hook=_fake_quant_hook)[-1]
            cos = torch.nn.functional.cosine_similarity(lg[i].float(), want, dim=0)
            assert float(cos) > 0.99, (step, i, float(cos))
        nxt = torch.argmax(lg, -1)
        seqs = [torch.cat([s, nxt[i:i + 1]]) for i, s in enumerate(seqs)]
        lg = ex.forward([(n, 1) for n in names], nxt)
    # the hook is off by default
    assert torch.equal(reference_forward([w], seqs[0]), reference_forward([w], seqs[0], kv_hook=None))


def test_executor_page_count_and_unsupported_models():
    cfg = resolve_model("tiny-llama")
    w = random_stage_weights(cfg, 0, 2, has_embed=False, has_head=False, device="cpu", dtype=torch.float32, seed=1)
    kw = dict(dtype=torch.float32, kv_cache_bytes=1 << 20, max_sessions=64, max_seq_len=2048)
    bf = StageExecutor(cfg, w, "cpu", **kw)
    f8 = StageExecutor(cfg, w, "cpu", kv_cache_dtype="fp8", **kw)
    D = cfg.head_dim
    per_page = 2 * 2 * cfg.num_key_value_heads * 64
    assert bf.kv_cache_dtype == "bf16" and bf.cache.num_pages == (1 << 20) // (per_page * D * 2)
    assert f8.cache.num_pages == (1 << 20) // (per_page * (D + 1))
    assert f8.sessions.cache_tokens_left() > 1.9 * bf.sessions.cache_tokens_left()
    with pytest.raises(ValueError):
        StageExecutor(cfg, w, "cpu", kv_cache_dtype="int8", **kw)
    gcfg = resolve_model("tiny-gpt2")
    gw = random_stage_weights(gcfg, 0, 1, has_embed=True, has_head=True, device="cpu", dtype=torch.float32)
    with pytest.raises(ValueError, match="GPT-2"):
        StageExecutor(gcfg, gw, "cpu", dtype=torch.float32, kv_cache_dtype="fp8")


# ------------------------------------------------------------------------------------- CLI, interface
def test_kv_cache_dtype_parser_and_executor_kwargs():
    argv = ["--model", "tiny-llama", "--splits", "1", "--stage", "1"]
    a = build_parser().parse_args(argv)
    assert a.kv_cache_dtype == "bf16" and "kv_cache_dtype" not in _executor_kwargs(a)
    a = build_parser().parse_args(argv + ["--kv_cache_dtype", "fp8"])
    assert a.kv_cache_dtype == "fp8" and _executor_kwargs(a)["kv_cache_dtype"] == "fp8"
    with pytest.raises(SystemExit):
        build_parser().parse_args(argv + ["--kv_cache_dtype", "int4"])


def test_sizing_takes_the_kv_dtype():
    cfg = resolve_model("llama2-7b")
    assert cfg.kv_bytes_per_token_per_layer(2) == 2 * 32 * 128 * 2
    assert cfg.kv_bytes_per_token_per_layer(2, "fp8") == 2 * 32 * 129
    with pytest.raises(ValueError):
        cfg.kv_bytes_per_token_per_layer(2, "int4")
    assert kv_cache_bytes_per_block(cfg, 1000, kv_cache_dtype="fp8") * 256 == \
        kv_cache_bytes_per_block(cfg, 1000) * 129
    for free in (3 << 30, 6 << 30, 20 << 30):
        nb = auto_num_blocks(cfg, free_bytes=free, attn_cache_tokens=16384)
        nf = auto_num_blocks(cfg, free_bytes=free, attn_cache_tokens=16384, kv_cache_dtype="fp8")
        assert nf >= nb >= 1
    # 20 GiB free, 16K cache tokens: a block is 0.377 GiB of weights + 0.25 (bf16) / 0.126 (fp8) GiB of KV
    assert auto_num_blocks(cfg, free_bytes=20 << 30, attn_cache_tokens=16384, kv_cache_dtype="fp8") > \
        auto_num_blocks(cfg, free_bytes=20 << 30, attn_cache_tokens=16384)


def test_throughput_cache_key_carries_the_kv_dtype():
    from src.throughput_measurement import ThroughputCache

    cfg = resolve_model("tiny-llama")
    w = random_stage_weights(cfg, 0, 1, has_embed=False, has_head=False, device="cpu", dtype=torch.float32)
    kw = dict(dtype=torch.float32, kv_cache_bytes=1 << 20, max_sessions=2, max_seq_len=64)
    kb = ThroughputCache.key(StageExecutor(cfg, w, "cpu", **kw))
    kf = ThroughputCache.key(StageExecutor(cfg, w, "cpu", kv_cache_dtype="fp8", **kw))
    assert "kvfp8" in kf and "kv" not in kb.split("|")[-1] and kf.startswith(kb)


@pytest.mark.timeout(120)
def test_stage_server_with_fp8_kv_generates_and_announces_it():
    """``--kv_cache_dtype fp8`` on a stage server (CPU): ``rpc_info`` and the announcement carry the
    field, and the client's greedy tokens come out of the served span."""
    from src import main as M
    from src.comm.wire import Message
    from src.dht_utils import get_stage_key

    from .swarm_utils import ServerThread, client_args, server_argv

    model, cut = "tiny-llama", 2
    s1 = ServerThread(server_argv(model, str(cut), 1, extra="--kv_cache_dtype fp8")).wait()
    try:
        assert s1.srv.ex.kv_cache_dtype == "fp8" and s1.srv.ex.cache.is_fp8
        info = s1.srv.loop.run(s1.srv.handler.rpc_info(Message({}, [])), timeout=10)
        assert info.metadata["kv_cache_dtype"] == "fp8"
        rec = s1.dht.get(get_stage_key(1), latest=True)
        assert "kv_cache_dtype" in repr(rec.value) and "fp8" in repr(rec.value)
        args = client_args(model, str(cut), s1.addr, "--max_new_tokens 6 --temperature 0")
        gen = M.run_rank0(args, torch.device("cpu"), [cut])
    finally:
        s1.close()
    assert len(gen) == 6
