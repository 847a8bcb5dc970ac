"""fp8 KV cache on the GPU: the quantizing KV-write kernel and the fp8 form of the flash-decoding
kernel (csrc/rope_kv.hip, csrc/attention.hip, csrc/kv_f8.h) against the bf16 kernels and the row rule
``ops.quant_kv_fp8``, bit for bit where the operands are equal; the executor on an fp8 cache."""
import math

import pytest
import torch

from src import ops
from src.models.config import resolve_model
from src.models.reference_model import reference_forward
from src.models.weights import random_stage_weights
from src.ops import reference as ref
from src.runtime.executor import StageExecutor

pytestmark = pytest.mark.gpu
DEV = "cuda"
SENT = 0xA5  # sentinel byte the caches are pre-filled with


@pytest.fixture(scope="module", autouse=True)
def _native():
    assert ops.load_library(), "HIP kernel library must load on the GPU box"
    torch.manual_seed(0)


def bf(x):
    return x.to(torch.bfloat16)


def _sentinel_cache(P, nkv, ps, D):
    return ops.KVF8(torch.full((P, nkv, ps, D), SENT, dtype=torch.uint8, device=DEV),
                    torch.full((P, nkv, ps), SENT, dtype=torch.uint8, device=DEV))


def _rows_of(cache, slots, ps):
    """cache [P, nkv, ps, ...] -> the rows [n, nkv, ...] at ``slots``."""
    return cache[slots // ps, :, slots % ps]


# ------------------------------------------------------------------------------------- write kernel
@pytest.mark.parametrize("nh,nkv,D", [(32, 32, 128), (8, 2, 128), (12, 12, 64)])
def test_rope_kv_write_f8_is_the_bf16_write_then_the_row_rule(nh, nkv, D):
    T, P, ps = 19, 16, 64
    qkv = bf(torch.randn(T, (nh + 2 * nkv) * D, device=DEV))
    view = qkv.view(T, nh + 2 * nkv, D)
    view[3, nh + nkv + 1] = 0          # one all-zero v head
    view[5] *= 300                     # one large row
    view[7] *= 1e-3                    # one small row
    pos = torch.randint(0, 500, (T,), device=DEV)
    slots = torch.randperm(P * ps, device=DEV)[:T]
    slots[11] = -1
    cos, sin = ops.rope_cos_sin(D, 2048, 10000.0, DEV)
    kb = torch.zeros(P, nkv, ps, D, dtype=torch.bfloat16, device=DEV)
    vb = torch.zeros_like(kb)
    q_bf = qkv.clone()
    ops.rope_kv_write(q_bf, pos, cos, sin, kb, vb, slots, nh, nkv)
    kf, vf = _sentinel_cache(P, nkv, ps, D), _sentinel_cache(P, nkv, ps, D)
    q_f8 = qkv.clone()
    ops.rope_kv_write(q_f8, pos, cos, sin, kf, vf, slots, nh, nkv)
    assert torch.equal(q_f8, q_bf)
    ok = slots[slots >= 0]
    for cf, cb in ((kf, kb), (vf, vb)):
        qc, qe = ops.quant_kv_fp8(_rows_of(cb, ok, ps))
        assert torch.equal(_rows_of(cf.codes, ok, ps), qc)
        assert torch.equal(_rows_of(cf.scales, ok, ps), qe)
        # every other byte still holds the sentinel
        codes, scales = cf.codes.clone(), cf.scales.clone()
        codes[ok // ps, :, ok % ps] = SENT
        scales[ok // ps, :, ok % ps] = SENT
        assert bool((codes == SENT).all()) and bool((scales == SENT).all())
    # the zero v head (token 3, kv head 1): unit scale, zero codes
    assert int(_rows_of(vf.scales, slots[3:4], ps)[0, 1]) == 127
    assert int(_rows_of(vf.codes, slots[3:4], ps)[0, 1].sum()) == 0


# ------------------------------------------------------------------------- attention without RoPE
def _attn_case(nh, nkv, D, ctxs, ps=64, multi_q=False):
    """An fp8 cache of random rows, the bf16 cache of its dequantized values, and queries."""
    S = len(ctxs)
    maxp = max(math.ceil(max(c, 1) / ps) for c in ctxs) + 1
    P = S * maxp + 3
    kf = ops.KVF8.from_dense(bf(torch.randn(P, nkv, ps, D, device=DEV)))
    vf = ops.KVF8.from_dense(bf(torch.randn(P, nkv, ps, D, device=DEV) * torch.rand(P, nkv, ps, 1, device=DEV) * 4))
    bt = torch.randperm(P, device=DEV)[: S * maxp].view(S, maxp).to(torch.int32)
    if multi_q:
        q_seq = torch.cat([torch.full((c,), i, dtype=torch.int32) for i, c in enumerate(ctxs)]).to(DEV)
        q_ctx = torch.cat([torch.arange(1, c + 1, dtype=torch.int32) for c in ctxs]).to(DEV)
    else:
        q_seq = torch.arange(S, dtype=torch.int32, device=DEV)
        q_ctx = torch.tensor(ctxs, dtype=torch.int32, device=DEV)
    q = bf(torch.randn(q_seq.numel(), (nh + 2 * nkv) * D, device=DEV))
    return q, kf, vf, kf.dequant(), vf.dequant(), bt, q_seq, q_ctx


_SHAPES = [(32, 32, 128), (32, 8, 128), (64, 8, 128), (12, 12, 64), (8, 2, 64)]


@pytest.mark.parametrize("nh,nkv,D", _SHAPES)
@pytest.mark.parametrize("ctxs", [[1, 5, 64, 200], [1000, 3]])
def test_paged_attention_f8_equals_bf16_kernel_on_dequantized_cache(nh, nkv, D, ctxs):
    q, kf, vf, kd, vd, bt, q_seq, q_ctx = _attn_case(nh, nkv, D, ctxs)
    scale = 1 / math.sqrt(D)
    out = ops.paged_attention(q, kf, vf, bt, q_seq, q_ctx, nh, nkv, scale)
    want = ops.paged_attention(q, kd, vd, bt, q_seq, q_ctx, nh, nkv, scale)
    assert torch.equal(out, want)
    o_ref = ref.paged_attention(q.float(), kd.float(), vd.float(), bt, q_seq, q_ctx, nh, nkv, scale)
    torch.testing.assert_close(out.float(), o_ref.float(), atol=2e-2, rtol=2e-2)


@pytest.mark.parametrize("nh,nkv,D", _SHAPES)
@pytest.mark.parametrize("inlaunch", [False, True])
@pytest.mark.parametrize("packed", [False, True])
def test_paged_attention_f8_split_k_combine_and_packed(nh, nkv, D, inlaunch, packed, monkeypatch):
    monkeypatch.setattr(ops, "ATTN_INLAUNCH_REDUCE", inlaunch)
    q, kf, vf, kd, vd, bt, q_seq, q_ctx = _attn_case(nh, nkv, D, [1, 5, 64, 200])
    scale = 1 / math.sqrt(D)
    kw = dict(part_size=64, num_parts=8, packed=packed)
    out = ops.paged_attention(q, kf, vf, bt, q_seq, q_ctx, nh, nkv, scale, **kw)
    want = ops.paged_attention(q, kd, vd, bt, q_seq, q_ctx, nh, nkv, scale, **kw)
    T = q.shape[0]
    if packed:
        out, want = ref.unpack_act(out, T, nh * D), ref.unpack_act(want, T, nh * D)
    assert torch.equal(out, want)
    o_ref = ref.paged_attention(q.float(), kd.float(), vd.float(), bt, q_seq, q_ctx, nh, nkv, scale)
    torch.testing.assert_close(out.float(), o_ref.float(), atol=2e-2, rtol=2e-2)


@pytest.mark.parametrize("nh,nkv,D", _SHAPES)
def test_paged_attention_f8_multi_query_causal(nh, nkv, D):
    q, kf, vf, kd, vd, bt, q_seq, q_ctx = _attn_case(nh, nkv, D, [70, 9], multi_q=True)
    q_ctx[-1] = 0  # a padded row: zeros
    scale = 1 / math.sqrt(D)
    out = ops.paged_attention(q, kf, vf, bt, q_seq, q_ctx, nh, nkv, scale)
    want = ops.paged_attention(q, kd, vd, bt, q_seq, q_ctx, nh, nkv, scale)
    assert torch.equal(out, want)
    assert torch.count_nonzero(out[-1]) == 0
    o_ref = ref.paged_attention(q.float(), kd.float(), vd.float(), bt, q_seq, q_ctx, nh, nkv, scale)
    torch.testing.assert_close(out.float(), o_ref.float(), atol=2e-2, rtol=2e-2)


# ------------------------------------------------------------------------------------ fused decode
def _fused_case(nh, nkv, D, ctxs, ps=64):
    q, kf, vf, kd, vd, bt, q_seq, q_ctx = _attn_case(nh, nkv, D, [max(c, 1) for c in ctxs], ps=ps)
    pad = [i for i, c in enumerate(ctxs) if c == 0]
    for i in pad:
        q_ctx[i] = 0
    pos = (q_ctx.long() - 1).clamp(min=0)
    slots = torch.stack([bt[i, int(p) // ps].long() * ps + int(p) % ps for i, p in enumerate(pos.tolist())])
    for i in pad:
        slots[i] = -1
    return q, kf, vf, kd, vd, bt, q_seq, q_ctx, pos, slots


def _check_fused_write(kf, vf, k0, v0, kb, vb, slots, ps):
    """The fp8 kernel wrote quant_kv_fp8 of the rows the bf16 fused kernel wrote (``kb`` / ``vb``) at
    ``slots`` and nothing else (``k0`` / ``v0``: the fp8 caches before the launch)."""
    ok = slots[slots >= 0]
    for cf, c0, cb in ((kf, k0, kb), (vf, v0, vb)):
        qc, qe = ops.quant_kv_fp8(_rows_of(cb, ok, ps))
        assert torch.equal(_rows_of(cf.codes, ok, ps), qc)
        assert torch.equal(_rows_of(cf.scales, ok, ps), qe)
        codes, scales = cf.codes.clone(), cf.scales.clone()
        codes[ok // ps, :, ok % ps] = _rows_of(c0.codes, ok, ps)
        scales[ok // ps, :, ok % ps] = _rows_of(c0.scales, ok, ps)
        assert torch.equal(codes, c0.codes) and torch.equal(scales, c0.scales)


@pytest.mark.parametrize("nh,nkv,D", [(32, 32, 128), (32, 8, 128), (12, 12, 64)])
@pytest.mark.parametrize("parts", [None, (64, 8)])
@pytest.mark.parametrize("packed", [False, True])
def test_paged_attention_rope_f8_fused(nh, nkv, D, parts, packed):
    """The fused fp8 decode step: qkv untouched; the new token written as quant_kv_fp8 of what the
    bf16 fused kernel writes, nothing else touched; the output is attention over the POST-write fp8
    cache (the new token seen through its dequantized values); the padded row outputs zeros."""
    ctxs, ps = [1, 5, 64, 200, 0], 64
    q, kf, vf, kd, vd, bt, q_seq, q_ctx, pos, slots = _fused_case(nh, nkv, D, ctxs, ps)
    cos, sin = ops.rope_cos_sin(D, 2048, 10000.0, DEV)
    scale = 1 / math.sqrt(D)
    kw = dict(part_size=parts[0], num_parts=parts[1]) if parts else dict(max_ctx=max(ctxs))
    k0, v0 = ops.KVF8(kf.codes.clone(), kf.scales.clone()), ops.KVF8(vf.codes.clone(), vf.scales.clone())
    q_in = q.clone()
    o1 = ops.paged_attention_rope(q, kf, vf, bt, q_seq, q_ctx, pos, cos, sin, slots, nh, nkv, scale, packed=packed, **kw)
    assert torch.equal(q, q_in), "fused op must not modify qkv"
    # the bf16 fused kernel on a bf16 copy of the dequantized cache: the rows this step writes
    kb, vb = kd.clone(), vd.clone()
    ops.paged_attention_rope(q, kb, vb, bt, q_seq, q_ctx, pos, cos, sin, slots, nh, nkv, scale, packed=packed, **kw)
    _check_fused_write(kf, vf, k0, v0, kb, vb, slots, ps)
    # two bf16 kernels over the dequantized post-write fp8 cache
    q2, k2, v2 = q.clone(), kf.dequant(), vf.dequant()
    ops.rope_kv_write(q2, pos, cos, sin, torch.empty_like(k2), torch.empty_like(v2), slots, nh, nkv)
    o2 = ops.paged_attention(q2, k2, v2, bt, q_seq, q_ctx, nh, nkv, scale, packed=packed, **kw)
    T = q.shape[0]
    if packed:
        o1, o2 = ref.unpack_act(o1, T, nh * D), ref.unpack_act(o2, T, nh * D)
    torch.testing.assert_close(o1.float(), o2.float(), atol=2e-2, rtol=2e-2)
    assert torch.count_nonzero(o1[-1]) == 0


def test_paged_attention_rope_f8_through_the_qkv_fold():
    """q / k / v read from the qkv GEMM's split-K slabs (``qkv_part``) == the same step on the bf16
    qkv rows the reduce launch stores: output and cache bit for bit."""
    nh, nkv, D, M, K, ps = 32, 32, 128, 16, 1024, 64
    N = (nh + 2 * nkv) * D
    assert ops.rwk_split(M, N, K, False) > 0
    g = torch.Generator(device=DEV).manual_seed(5)
    ctxs = torch.randint(1, 96, (M,), generator=g, device=DEV).to(torch.int32)
    P = 2 * M + 3
    dense = bf(torch.randn(P, nkv, ps, D, device=DEV, generator=g) * 0.5)
    bt = torch.randperm(P, device=DEV)[: 2 * M].view(M, 2).to(torch.int32)
    pos = ctxs.long() - 1
    slots = torch.stack([bt[i, int(p) // ps].long() * ps + int(p) % ps for i, p in enumerate(pos.tolist())])
    x = bf(torch.randn(M, K, device=DEV, generator=g) * 0.7)
    ss = ops.norm_stats_buffer(DEV)[0]
    ss.zero_()
    ss[0, :M] = torch.round((x.float() ** 2).sum(1) * 2.0 ** 20).long()
    wp = ops.pack_weight(bf(torch.randn(N, K, device=DEV, generator=g) * 0.03))
    xp = ops.pack_act(x)
    ops.set_gemm_sk("rwk")
    try:
        qkv = ops.linear(xp, None, wp=wp, a_rows=M, ss_in=ss, eps=1e-5)
    finally:
        ops.set_gemm_sk("auto")
    dummy = torch.full_like(qkv, float("nan"))
    part = ops.linear_partials(xp, M, wp=wp, out=dummy)
    cos, sin = ops.rope_cos_sin(D, 2048, 10000.0, DEV)
    q_seq = torch.arange(M, dtype=torch.int32, device=DEV)
    res = []
    for rows, qp in ((qkv, None), (dummy, (part, ss, 1.0 / K, 1e-5))):
        kf, vf = ops.KVF8.from_dense(dense), ops.KVF8.from_dense(dense * 2)
        o = ops.paged_attention_rope(rows, kf, vf, bt, q_seq, ctxs, pos, cos, sin, slots, nh, nkv,
                                     1 / math.sqrt(D), max_ctx=96, packed=True, qkv_part=qp)
        res.append((ops.unpack_act(o, M, nh * D).clone(), kf, vf))
    (o1, k1, v1), (o2, k2, v2) = res
    assert torch.equal(o1, o2) and bool(torch.isfinite(o1.float()).all())
    for a, b in ((k1, k2), (v1, v2)):
        assert torch.equal(a.codes, b.codes) and torch.equal(a.scales, b.scales)


# ------------------------------------------------------------------ the bf16-only attention kernels
def test_mfma_and_fa_attention_reject_an_fp8_cache():
    nh, nkv, D = 32, 8, 128
    q, kf, vf, kd, vd, bt, q_seq, q_ctx = _attn_case(nh, nkv, D, [5, 9])
    qb = torch.from_numpy(ops.query_blocks([1, 1], nh // nkv)).to(DEV)
    cos, sin = ops.rope_cos_sin(D, 64, 10000.0, DEV)
    pos, slots = q_ctx.long() - 1, torch.zeros(2, dtype=torch.long, device=DEV)
    with pytest.raises(NotImplementedError, match="fp8 KV"):
        ops.attention_mfma(q, kf, vf, bt, q_seq, q_ctx, qb, nh, nkv, 1.0)
    with pytest.raises(NotImplementedError, match="fp8 KV"):
        ops.attention_fa(q, kf, vf, bt, q_seq, q_ctx, qb, nh, nkv, 1.0)
    with pytest.raises(NotImplementedError, match="fp8 KV"):
        ops.attention_mfma_rope(q, kf, vf, bt, q_seq, q_ctx, qb, pos, cos, sin, slots, nh, nkv, 1.0)
    # and the bindings themselves refuse byte pages where they read bf16 ones
    out = torch.empty(2, nh * D, dtype=torch.bfloat16, device=DEV)
    ws = ops.attention_workspace(2, nh, D, 1, DEV)
    with pytest.raises(RuntimeError, match="bf16"):
        torch.ops.mpamd.paged_attention(q, kf.codes, vf.codes, bt, q_seq, q_ctx, out, ws, nh, nkv, 1.0, 64, 1, 0, None)
    with pytest.raises(RuntimeError, match="bf16"):
        torch.ops.mpamd.attention_mfma(q, kf.codes, vf.codes, bt, q_seq, q_ctx, qb, out, ws, nh, nkv, 1.0, 128, 1, 0,
                                       None)
    with pytest.raises(RuntimeError, match="scales"):  # scales of another page_size
        torch.ops.mpamd.paged_attention(q, kf.codes, vf.codes, bt, q_seq, q_ctx, out, ws, nh, nkv, 1.0, 64, 1, 0, None,
                                        k_scale=kf.scales[:, :, :32].contiguous(),
                                        v_scale=vf.scales[:, :, :32].contiguous())


# ----------------------------------------------------------------------------------------- executor
def _fake_quant_hook(k, v):
    return ops.fake_quant_kv_fp8(k), ops.fake_quant_kv_fp8(v)


def _lens(B, long_at=3):
    lens = [5 + (7 * i) % 23 for i in range(B)]
    lens[long_at] = 70  # crosses a 64-token page
    return lens


def _run(ex, cfg, B=17, steps=3, chunked=False):
    g = torch.Generator().manual_seed(11)
    seqs = [torch.randint(0, cfg.vocab_size, (n,), generator=g).to(DEV) for n in _lens(B)]
    names = [f"s{i}" for i in range(B)]
    if chunked:  # 3 tokens of every prompt, then the rest: the second step is a chunked prefill
        ex.forward([(n, 3) for n in names], torch.cat([s[:3] for s in seqs]))
        lg = ex.forward([(n, len(s) - 3) for n, s in zip(names, seqs)], torch.cat([s[3:] for s in seqs]))
    else:
        lg = ex.forward([(n, len(s)) for n, s in zip(names, seqs)], torch.cat(seqs))
    outs = [lg.float().clone()]
    for _ in range(steps):
        nxt = torch.argmax(lg.float(), -1)
        seqs = [torch.cat([s, nxt[i:i + 1]]) for i, s in enumerate(seqs)]
        lg = ex.forward([(n, 1) for n in names], nxt)
        outs.append(lg.float().clone())
    torch.cuda.synchronize()
    return outs, seqs


def _check_oracle(wd, outs, seqs, rows):
    for i in rows:
        want = reference_forward([wd], seqs[i], kv_hook=_fake_quant_hook)[-1].float()
        cos = torch.nn.functional.cosine_similarity(outs[-1][i], want, dim=0)
        assert float(cos) > 0.99, (i, float(cos))


def _count_mfma(monkeypatch):
    calls = []
    for name in ("attention_mfma", "attention_mfma_rope", "attention_fa"):
        monkeypatch.setattr(ops, name, lambda *a, _n=name, **k: calls.append(_n))
    return calls


@pytest.mark.parametrize("model", ["small-llama", "tiny-llama"])
@pytest.mark.parametrize("fused", ["1", "0"])
def test_executor_fp8_kv_graphs_and_oracle(model, fused, monkeypatch):
    """17 ragged sessions (one past a page), prefill + 3 decode steps on an fp8 cache: hipGraphs on
    == off bit for bit, logits track the fake-quantized oracle, no MFMA / FA2 attention launch."""
    monkeypatch.setenv("MPAMD_FUSED_NORM", fused)
    calls = _count_mfma(monkeypatch)
    cfg = resolve_model(model)
    w = random_stage_weights(cfg, 0, cfg.num_hidden_layers, has_embed=True, has_head=True, device=DEV, seed=3)
    outs = {}
    for g in (False, True):
        ex = StageExecutor(cfg, w, DEV, kv_cache_bytes=64 << 20, max_sessions=32, max_seq_len=128, use_graphs=g,
                           kv_cache_dtype="fp8")
        assert ex.cache.k.dtype == torch.uint8 and ex.cache.k_scale.dtype == torch.uint8 and not ex.gqa_decode_mfma
        outs[g] = _run(ex, cfg)
        assert ex.last_graphed == g
    for a, b in zip(outs[False][0], outs[True][0]):
        assert torch.equal(a, b)
    assert not calls
    _check_oracle(w, *outs[True], rows=(0, 3, 16))


def test_executor_fp8_kv_chunked_prefill(monkeypatch):
    calls = _count_mfma(monkeypatch)
    cfg = resolve_model("small-llama")
    w = random_stage_weights(cfg, 0, cfg.num_hidden_layers, has_embed=True, has_head=True, device=DEV, seed=3)
    kw = dict(kv_cache_bytes=64 << 20, max_sessions=32, max_seq_len=128, use_graphs=False, kv_cache_dtype="fp8")
    one, seqs = _run(StageExecutor(cfg, w, DEV, **kw), cfg)
    two, seqs2 = _run(StageExecutor(cfg, w, DEV, **kw), cfg, chunked=True)
    assert not calls
    _check_oracle(w, one, seqs, rows=(3, 9))
    _check_oracle(w, two, seqs2, rows=(3, 9))


@pytest.mark.parametrize("quant", ["fp8", "mxfp4"])
def test_executor_fp8_kv_under_quantized_weights(quant, monkeypatch):
    calls = _count_mfma(monkeypatch)
    cfg = resolve_model("small-llama")
    w = random_stage_weights(cfg, 0, cfg.num_hidden_layers, has_embed=True, has_head=True, device=DEV, seed=3,
                             quant_type=quant)
    # the oracle's weights: the dequantized projections (unit norms: nothing to fold)
    wd = random_stage_weights(cfg, 0, cfg.num_hidden_layers, has_embed=True, has_head=True, device=DEV, seed=3,
                              dtype=torch.float32)
    for L, Ld in zip(w.layers, wd.layers):
        assert bool((L.input_norm == 1).all()) and bool((L.post_norm == 1).all())
        for name in L.PROJ:
            setattr(Ld, name, L.dense(name, torch.float32))
    ex = StageExecutor(cfg, w, DEV, kv_cache_bytes=64 << 20, max_sessions=32, max_seq_len=128, kv_cache_dtype="fp8")
    assert ex.quant_type == quant and ex.cache.is_fp8
    outs, seqs = _run(ex, cfg)
    assert not calls and bool(torch.isfinite(outs[-1]).all())
    _check_oracle(wd, outs, seqs, rows=(0, 3, 16))


def test_executor_fp8_kv_page_count():
    cfg = resolve_model("small-llama")
    w = random_stage_weights(cfg, 0, 2, has_embed=False, has_head=False, device=DEV, seed=3)
    kw = dict(kv_cache_bytes=8 << 20, max_sessions=256, max_seq_len=2048, use_graphs=False)
    nb = StageExecutor(cfg, w, DEV, **kw).cache.num_pages
    nf = StageExecutor(cfg, w, DEV, kv_cache_dtype="fp8", **kw).cache.num_pages
    D = cfg.head_dim
    per = 2 * 2 * cfg.num_key_value_heads * 64
    assert nb == (8 << 20) // (per * 2 * D) and nf == (8 << 20) // (per * (D + 1))
    assert nf == nb * 2 * D // (D + 1)
