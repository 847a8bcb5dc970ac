"""The MFMA GQA decode kernel on an fp8 KV cache (csrc/attention_mfma.hip F8 form, ops.attention_mfma_f8 /
ops.attention_mfma_rope_f8): it converts the e4m3 codes exactly and then does the bf16 kernel's own
arithmetic, so it is compared bit for bit with the bf16 kernel on the dequantized cache wherever the
operands are equal, with the row rule ``ops.quant_kv_fp8`` for what it writes, and through the
closed-form probes of tests/attn_probe.py for WHICH keys it reads (0xFF page tails included); then
the executor on an fp8 cache with a GQA model, hipGraphs on and off, and the MPAMD_KV_FP8_MFMA switch.

Largest |out - closed form| measured on an MI355X over all probes of all cases, next to the derived
bound 2^-6 = 0.015625 (``pytest -s`` prints them again as PROBE_DEV lines):
    attention_mfma_f8 decode                                                    0.003795
    attention_mfma_rope_f8                                                      0.003795
(the bf16 rounding of the output alone, as for the bf16 kernel: test_attention_probe_gpu.py)."""
import dataclasses
import functools
import math

import pytest
import torch

from src import ops
from src.models.config import resolve_model
from src.models.reference_model import reference_forward
from src.models.weights import random_stage_weights
from src.ops import reference as ref
from src.runtime.executor import StageExecutor
from tests import attn_probe as ap

pytestmark = pytest.mark.gpu
DEV = "cuda"
PS = 64

_SEEN = {}  # kernel -> largest deviation from the closed form in this run


@pytest.fixture(scope="module", autouse=True)
def _native():
    assert ops.load_library(), "HIP kernel library must load on the GPU box"
    torch.manual_seed(0)
    yield
    for k, v in sorted(_SEEN.items()):
        print(f"\nPROBE_DEV {k} {v:.6f}", end="")


def _note(kernel, dev):
    _SEEN[kernel] = max(_SEEN.get(kernel, 0.0), dev)


def bf(x):
    return x.to(torch.bfloat16)


def _copy(c):
    return ops.KVF8(c.codes.clone(), c.scales.clone())


def _rows_of(cache, slots, ps):
    """cache [P, nkv, ps, ...] -> the rows [n, nkv, ...] at ``slots``."""
    return cache[slots // ps, :, slots % ps]


def _qblocks(T, nrep):
    qb = torch.from_numpy(ops.query_blocks([1] * T, nrep)).to(DEV)
    assert qb.shape == (2, T)
    return qb


# (nh, nkv, D): HB 4, 8, 16 at D 128; HB 4 and 16 at D 64
SHAPES = [(32, 8, 128), (64, 8, 128), (32, 2, 128), (8, 2, 64), (16, 1, 64)]


def _attn_case(nh, nkv, D, ctxs, ps=PS):
    """An fp8 cache of random rows, the bf16 cache of its dequantized values, and one query per
    sequence; a context of 0 is a padded row (its cache still holds a token)."""
    S = len(ctxs)
    maxp = max(math.ceil(max(c, 1) / ps) for c in ctxs) + 1
    P = S * maxp + 3
    kf = ops.KVF8.from_dense(bf(torch.randn(P, nkv, ps, D, device=DEV)))
    vf = ops.KVF8.from_dense(bf(torch.randn(P, nkv, ps, D, device=DEV) * torch.rand(P, nkv, ps, 1, device=DEV) * 4))
    bt = torch.randperm(P, device=DEV)[: S * maxp].view(S, maxp).to(torch.int32)
    q_seq = torch.arange(S, dtype=torch.int32, device=DEV)
    q_ctx = torch.tensor(ctxs, dtype=torch.int32, device=DEV)
    q = bf(torch.randn(S, (nh + 2 * nkv) * D, device=DEV))
    return q, kf, vf, kf.dequant(), vf.dequant(), bt, q_seq, q_ctx


# ------------------------------------------------------------------------- attention without RoPE
@pytest.mark.parametrize("nh,nkv,D", SHAPES)
@pytest.mark.parametrize("ctxs", [[1, 5, 64, 200], [1000, 3]])
def test_attention_mfma_f8_equals_bf16_kernel_on_dequantized_cache(nh, nkv, D, ctxs):
    ctxs = ctxs + [0]  # one padded row: zeros
    q, kf, vf, kd, vd, bt, q_seq, q_ctx = _attn_case(nh, nkv, D, ctxs)
    T, n, scale = len(ctxs), max(ctxs), 1 / math.sqrt(D)
    qb = _qblocks(T, nh // nkv)
    o_ref = ref.paged_attention(q.float(), kd.float(), vd.float(), bt, q_seq, q_ctx, nh, nkv, scale).float()
    for part in ({}, dict(part_size=128 * math.ceil(n / 128), num_parts=1),
                 dict(part_size=128, num_parts=math.ceil(n / 128)), dict(part_size=256, num_parts=math.ceil(n / 256))):
        for packed in (False, True):
            kw = dict(packed=packed, **part)
            out = ops.attention_mfma_f8(q, kf, vf, bt, q_seq, q_ctx, qb, nh, nkv, scale, **kw)
            want = ops.attention_mfma(q, kd, vd, bt, q_seq, q_ctx, qb, nh, nkv, scale, **kw)
            if packed:
                out, want = ref.unpack_act(out, T, nh * D), ref.unpack_act(want, T, nh * D)
            assert torch.equal(out, want), kw
            assert torch.count_nonzero(out[-1]) == 0, kw
            torch.testing.assert_close(out.float(), o_ref, atol=2e-2, rtol=2e-2)


# ------------------------------------------------------------------------------------ fused decode
ROPE_CTXS = [1, 5, 64, 65, 200, 0]  # the last: a padded row, slots = -1, output zeros


def _fused_case(nh, nkv, D, ctxs, ps=PS):
    q, kf, vf, kd, vd, bt, q_seq, q_ctx = _attn_case(nh, nkv, D, ctxs, ps=ps)
    pos = (q_ctx.long() - 1).clamp(min=0)
    slots = torch.stack([bt[i, int(p) // ps].long() * ps + int(p) % ps for i, p in enumerate(pos.tolist())])
    for i, c in enumerate(ctxs):
        if c == 0:
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


@pytest.mark.parametrize("nh,nkv,D", SHAPES)
@pytest.mark.parametrize("parts", [None, (128, 2)])
def test_attention_mfma_rope_f8_exact_case(nh, nkv, D, parts):
    """Identity rotary table and new k / v rows that survive quantization: every operand of the fp8
    kernel equals the bf16 kernel's, so output and the cache after the launch are equal bit for bit."""
    q, kf, vf, kd, vd, bt, q_seq, q_ctx, pos, slots = _fused_case(nh, nkv, D, ROPE_CTXS)
    T, scale = q.shape[0], 1 / math.sqrt(D)
    view = q.view(T, nh + 2 * nkv, D)
    view[:, nh:] = ops.fake_quant_kv_fp8(view[:, nh:].clone())
    cos = torch.ones(256, D // 2, dtype=torch.float32, device=DEV)
    sin = torch.zeros_like(cos)
    qb = _qblocks(T, nh // nkv)
    kw = dict(part_size=parts[0], num_parts=parts[1]) if parts else {}
    q_in = q.clone()
    out = ops.attention_mfma_rope_f8(q, kf, vf, bt, q_seq, q_ctx, qb, pos, cos, sin, slots, nh, nkv, scale, **kw)
    assert torch.equal(q, q_in), "the fused op must not modify qkv"
    kb, vb = kd.clone(), vd.clone()  # bf16 copies of the dequantized pre-write cache
    want = ops.attention_mfma_rope(q, kb, vb, bt, q_seq, q_ctx, qb, pos, cos, sin, slots, nh, nkv, scale, **kw)
    assert torch.equal(out, want)
    assert torch.count_nonzero(out[-1]) == 0
    assert not torch.equal(kb, kd) and not torch.equal(vb, vd)  # the bf16 launch wrote the new tokens
    assert torch.equal(kf.dequant(), kb) and torch.equal(vf.dequant(), vb)


@pytest.mark.parametrize("nh,nkv,D", SHAPES)
@pytest.mark.parametrize("parts", [None, (128, 2)])
def test_attention_mfma_rope_f8_real_rotary_table(nh, nkv, D, parts):
    """The new token written as quant_kv_fp8 of what the bf16 fused kernel writes, nothing else
    touched; the output is attention over the POST-write fp8 cache (the only difference to the
    unfused pair: the new token's score is summed on the VALU instead of the MFMA)."""
    q, kf, vf, kd, vd, bt, q_seq, q_ctx, pos, slots = _fused_case(nh, nkv, D, ROPE_CTXS)
    T, scale = q.shape[0], 1 / math.sqrt(D)
    cos, sin = ops.rope_cos_sin(D, 2048, 10000.0, DEV)
    qb = _qblocks(T, nh // nkv)
    kw = dict(part_size=parts[0], num_parts=parts[1]) if parts else {}
    k0, v0 = _copy(kf), _copy(vf)
    q_in = q.clone()
    o1 = ops.attention_mfma_rope_f8(q, kf, vf, bt, q_seq, q_ctx, qb, pos, cos, sin, slots, nh, nkv, scale, **kw)
    assert torch.equal(q, q_in), "the fused op must not modify qkv"
    kb, vb = kd.clone(), vd.clone()
    ops.attention_mfma_rope(q, kb, vb, bt, q_seq, q_ctx, qb, pos, cos, sin, slots, nh, nkv, scale, **kw)
    _check_fused_write(kf, vf, k0, v0, kb, vb, slots, PS)
    # the unfused pair on the same pre-write fp8 cache
    q2, k2, v2 = q.clone(), _copy(k0), _copy(v0)
    ops.rope_kv_write(q2, pos, cos, sin, k2, v2, slots, nh, nkv)
    o2 = ops.attention_mfma_f8(q2, k2, v2, bt, q_seq, q_ctx, qb, nh, nkv, scale, **kw)
    torch.testing.assert_close(o1.float(), o2.float(), atol=2e-2, rtol=2e-2)
    assert torch.count_nonzero(o1[-1]) == 0


# -------------------------------------------------------------------------------------- qkv fold
@pytest.mark.parametrize("nh,nkv,D", [(32, 8, 128), (64, 8, 128)])
@pytest.mark.parametrize("M", [1, 16])
def test_attention_mfma_rope_f8_through_the_qkv_fold(nh, nkv, D, M):
    """q / k / v read from the qkv GEMM's split-K slabs (``qkv_part``) == the same step on the bf16
    qkv rows the reduce launch stores: output, codes and scales bit for bit."""
    K, ps = 1024, PS
    N = (nh + 2 * nkv) * D
    assert ops.rwk_split(M, N, K, False) > 0
    g = torch.Generator(device=DEV).manual_seed(5 + M)
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
    dummy = torch.full_like(qkv, float("nan"))  # never read on the fold path
    part = ops.linear_partials(xp, M, wp=wp, out=dummy)
    assert torch.equal(ops.reduce_qkv_part((part, ss, 1.0 / K, 1e-5)), qkv)
    cos, sin = ops.rope_cos_sin(D, 2048, 10000.0, DEV)
    q_seq = torch.arange(M, dtype=torch.int32, device=DEV)
    qb = _qblocks(M, nh // nkv)
    res = []
    for rows, qp in ((qkv, None), (dummy, (part, ss, 1.0 / K, 1e-5))):
        kf, vf = ops.KVF8.from_dense(dense), ops.KVF8.from_dense(dense * 2)
        o = ops.attention_mfma_rope_f8(rows, kf, vf, bt, q_seq, ctxs, qb, pos, cos, sin, slots, nh, nkv,
                                       1 / math.sqrt(D), max_ctx=96, packed=True, qkv_part=qp)
        res.append((ops.unpack_act(o, M, nh * D).clone(), kf, vf))
    (o1, k1, v1), (o2, k2, v2) = res
    assert torch.equal(o1, o2) and bool(torch.isfinite(o1.float()).all())
    for a, b in ((k1, k2), (v1, v2)):
        assert torch.equal(a.codes, b.codes) and torch.equal(a.scales, b.scales)
    assert not torch.equal(k1.codes, ops.KVF8.from_dense(dense).codes)  # the new tokens were written


# ---------------------------------------------------------------------------------------- probes
PROBE_SHAPES = [(32, 8, 128), (16, 4, 128), (8, 2, 64), (64, 8, 128)]


@functools.lru_cache(maxsize=None)
def _decode(nh, nkv, D):
    return ap.decode_case(nh, nkv, D, rows=3 if nh <= 16 else 2)


@functools.lru_cache(maxsize=None)
def _rope(nh, nkv, D, quarter):
    return ap.rope_case(nh, nkv, D, quarter=quarter)


@pytest.mark.parametrize("nh,nkv,D", PROBE_SHAPES)
def test_attention_mfma_f8_decode_probes(nh, nkv, D):
    case = _decode(nh, nkv, D)
    a = case.to(DEV)
    kc, vc = case.f8(DEV)
    q, bt, q_seq, q_ctx = a["q"], a["block_tables"], a["q_seq"], a["q_ctx"]
    qb = _qblocks(case.T, nh // nkv)
    n = max(ap.DECODE_CTXS)
    for kw in ({}, dict(part_size=128 * math.ceil(n / 128), num_parts=1), dict(part_size=128, num_parts=math.ceil(n / 128)),
               dict(part_size=256, num_parts=math.ceil(n / 256)),
               dict(part_size=256, num_parts=math.ceil(n / 256), packed=True)):
        out = ops.attention_mfma_f8(q, kc, vc, bt, q_seq, q_ctx, qb, nh, nkv, case.scale, **kw)
        if kw.get("packed", False):
            out = ops.unpack_act(out, case.T, nh * D)
        _note("attention_mfma_f8 decode", ap.compare(out, case, f"attention_mfma_f8 decode {kw}"))


def _check_cache_after(case, kc, vc):
    """The new token's slot holds the new k / v bit for bit, every other slot is unchanged, and the
    poison bytes 0xFF are intact in codes and scales."""
    ok = ~case.poison[:, None, :, None].expand_as(case.k_after)
    for got, want, name in ((kc.dequant().cpu(), case.k_after, "k"), (vc.dequant().cpu(), case.v_after, "v")):
        assert torch.equal(got[ok], want[ok]), f"{name} cache after the launch"
        assert got[~ok].isnan().all(), f"{name} cache: a poisoned slot was written"
    pz = case.poison[:, None, :].expand_as(kc.scales.cpu())
    for c in (kc, vc):
        assert (c.codes.cpu()[pz] == 0xFF).all() and (c.scales.cpu()[pz] == 0xFF).all()


@pytest.mark.parametrize("nh,nkv,D", PROBE_SHAPES)
@pytest.mark.parametrize("quarter", [False, True])
@pytest.mark.parametrize("parts", [None, (128, 8), (256, 4)])
def test_attention_mfma_rope_f8_probes(nh, nkv, D, quarter, parts):
    case = _rope(nh, nkv, D, quarter)
    a = case.to(DEV)
    kc, vc = case.f8(DEV)
    q = a["q"]
    qb = _qblocks(case.T, nh // nkv)
    kw = dict(part_size=parts[0], num_parts=parts[1]) if parts else {}
    out = ops.attention_mfma_rope_f8(q, kc, vc, a["block_tables"], a["q_seq"], a["q_ctx"], qb, a["positions"], a["cos"],
                                     a["sin"], a["slots"], nh, nkv, case.scale, **kw)
    _note("attention_mfma_rope_f8", ap.compare(out, case, f"attention_mfma_rope_f8 {parts} quarter={quarter}"))
    assert torch.equal(q.cpu(), case.q), "the fused op must not modify qkv"
    _check_cache_after(case, kc, vc)


# ------------------------------------------------------------------------------------- refusals
def test_the_f8_bindings_refuse_what_the_kernel_does_not_cover():
    nh, nkv, D = 32, 8, 128
    q, kf, vf, kd, vd, bt, q_seq, q_ctx = _attn_case(nh, nkv, D, [5, 9])
    qb = _qblocks(2, nh // nkv)
    cos, sin = ops.rope_cos_sin(D, 64, 10000.0, DEV)
    pos, slots = q_ctx.long() - 1, torch.full((2,), -1, dtype=torch.long, device=DEV)
    out = torch.empty(2, nh * D, dtype=torch.bfloat16, device=DEV)
    ws = ops.attention_workspace(2, nh, D, 1, DEV)
    m = torch.ops.mpamd

    def plain(k, v, ks, vs, qb_=qb, nkv_=nkv):
        m.attention_mfma(q, k, v, bt, q_seq, q_ctx, qb_, out, ws, nh, nkv_, 1.0, 128, 1, 0, k_scale=ks, v_scale=vs)

    def rope(k, v, ks, vs, qb_=qb, nkv_=nkv):
        m.attention_mfma_rope(q, k, v, bt, q_seq, q_ctx, qb_, pos, cos, sin, slots, out, ws, nh, nkv_, 1.0,
                              128, 1, 0, k_scale=ks, v_scale=vs)

    half = kf.scales[:, :, :32].contiguous()
    for call in (plain, rope):
        call(kf.codes, vf.codes, kf.scales, vf.scales)  # the accepted form
        with pytest.raises(RuntimeError, match="uint8"):  # bf16 caches
            call(kd, vd, kf.scales, vf.scales)
        with pytest.raises(RuntimeError, match="scales"):  # scales of another page size
            call(kf.codes, vf.codes, half, half)
        with pytest.raises(RuntimeError, match="one query token per block"):  # fewer blocks than tokens
            call(kf.codes, vf.codes, kf.scales, vf.scales, qb_=qb[:, :1].contiguous())
    torch.cuda.synchronize()
    # nh / nkv = 2: caches of 16 kv heads
    k16 = ops.KVF8.from_dense(bf(torch.randn(4, 16, PS, D, device=DEV)))
    for call in (plain, rope):
        with pytest.raises(RuntimeError, match="group sizes"):
            call(k16.codes, k16.codes, k16.scales, k16.scales, nkv_=16)
    # the bf16 binding still refuses code pages
    with pytest.raises(RuntimeError, match="bf16"):
        m.attention_mfma(q, kf.codes, vf.codes, bt, q_seq, q_ctx, qb, out, ws, nh, nkv, 1.0, 128, 1, 0, None)


# ----------------------------------------------------------------------------------------- executor
def _gqa4():
    return dataclasses.replace(resolve_model("small-llama"), num_key_value_heads=1, name="small-llama-gqa4")


def _fake_quant_hook(k, v):
    return ops.fake_quant_kv_fp8(k), ops.fake_quant_kv_fp8(v)


def _lens(B, long_at=3):
    lens = [5 + (7 * i) % 23 for i in range(B)]
    lens[long_at] = 70  # crosses a 64-token page
    return lens


def _run(ex, cfg, B=17, steps=3):
    g = torch.Generator().manual_seed(11)
    seqs = [torch.randint(0, cfg.vocab_size, (n,), generator=g).to(DEV) for n in _lens(B)]
    names = [f"s{i}" for i in range(B)]
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


def _count_calls(monkeypatch):
    """Wrap (not replace) the MFMA / FA2 attention ops: name -> calls."""
    calls = {}
    for name in ("attention_mfma", "attention_mfma_rope", "attention_fa", "attention_mfma_f8", "attention_mfma_rope_f8"):
        real = getattr(ops, name)

        def wrapped(*a, _n=name, _real=real, **k):
            calls[_n] = calls.get(_n, 0) + 1
            return _real(*a, **k)

        monkeypatch.setattr(ops, name, wrapped)
    return calls


@pytest.mark.parametrize("fused", ["1", "0"])
def test_executor_fp8_kv_gqa_runs_the_mfma_f8_kernel(fused, monkeypatch):
    """17 ragged sessions (one past a page), prefill + 3 decode steps of a GQA-4 model on an fp8 cache:
    the decode steps run ops.attention_mfma_rope_f8 and none of the bf16 MFMA / FA2 ops, hipGraphs on
    == off bit for bit, logits track the fake-quantized oracle."""
    monkeypatch.setenv("MPAMD_FUSED_NORM", fused)
    monkeypatch.delenv("MPAMD_KV_FP8_MFMA", raising=False)
    calls = _count_calls(monkeypatch)
    cfg = _gqa4()
    assert cfg.num_attention_heads // cfg.num_key_value_heads == 4 and cfg.head_dim == 128
    w = random_stage_weights(cfg, 0, cfg.num_hidden_layers, has_embed=True, has_head=True, device=DEV, seed=3)
    outs = {}
    for g in (False, True):
        ex = StageExecutor(cfg, w, DEV, kv_cache_bytes=64 << 20, max_sessions=32, max_seq_len=128, use_graphs=g,
                           kv_cache_dtype="fp8")
        assert ex.cache.is_fp8 and ex.gqa_decode_mfma_f8 and not ex.gqa_decode_mfma
        outs[g] = _run(ex, cfg)
        assert ex.last_graphed == g
    for a, b in zip(outs[False][0], outs[True][0]):
        assert torch.equal(a, b)
    assert calls.get("attention_mfma_rope_f8", 0) >= 1
    assert not any(calls.get(n, 0) for n in ("attention_mfma", "attention_mfma_rope", "attention_fa")), calls
    _check_oracle(w, *outs[True], rows=(0, 3, 16))


def test_executor_fp8_kv_gqa_switch_restores_the_flash_decoding_kernel(monkeypatch):
    monkeypatch.setenv("MPAMD_KV_FP8_MFMA", "0")
    calls = _count_calls(monkeypatch)
    cfg = _gqa4()
    w = random_stage_weights(cfg, 0, cfg.num_hidden_layers, has_embed=True, has_head=True, device=DEV, seed=3)
    ex = StageExecutor(cfg, w, DEV, kv_cache_bytes=64 << 20, max_sessions=32, max_seq_len=128, kv_cache_dtype="fp8")
    assert ex.cache.is_fp8 and not ex.gqa_decode_mfma_f8 and not ex.gqa_decode_mfma
    outs, seqs = _run(ex, cfg)
    assert not calls, calls
    _check_oracle(w, outs, seqs, rows=(0, 3, 16))
