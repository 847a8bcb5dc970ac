"""The FA2 prefill kernel on an fp8 KV cache (csrc/attention_fa.hip F8 form, ops.attention_fa_f8): it
converts the e4m3 codes exactly while staging them into the LDS tiles and then does the bf16 kernel's
own arithmetic, so it is compared bit for bit with ``ops.attention_fa`` on the dequantized cache (rows
of very different scales inside every 64-token tile, 0xFF page tails), and through the closed-form
probes of tests/attn_probe.py for WHICH keys it reads; then the binding's refusals and the executor
on an fp8 cache (MHA and GQA-4), whole and chunked prompts, hipGraphs on and off, and the
MPAMD_KV_FP8_FA switch.

Largest |out - closed form| measured on an MI355X over all probes of all cases, next to the derived
bound 2^-6 = 0.015625 (``pytest -s`` prints it again as a PROBE_DEV line):
    attention_fa_f8                                                             0.008328
(the bf16 kernel's own figure, test_attention_probe_gpu.py: the bf16 rounding of the output and of P
in the numerator against an unrounded row sum l)."""
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
D = 128

_SEEN = {}  # kernel -> largest deviation from the closed form in this run


@pytest.fixture(scope="module", autouse=True)
def _native():
    assert ops.load_library(), "HIP kernel library must load on the GPU box"
    yield
    for k, v in sorted(_SEEN.items()):
        print(f"\nPROBE_DEV {k} {v:.6f}", end="")


def _note(kernel, dev):
    _SEEN[kernel] = max(_SEEN.get(kernel, 0.0), dev)


def bf(x):
    return x.to(torch.bfloat16)


# ----------------------------------------------------------------------------------- bit equality
PROMPTS = [((70, 9, 1, 33, 130), (0, 0, 0, 0, 0)), ((300, 17), (64, 5)), ((129, 256), (0, 63))]


@functools.lru_cache(maxsize=None)
def _eq_case(nh, nkv, ntoks, prefix):
    """An fp8 cache whose rows carry factors 2^-3 .. 2^3 (so the e8m0 scale bytes differ from row to row
    inside every 64-token tile), 0xFF codes and scales past every context to the end of its last page,
    the bf16 cache of its dequantized values (NaN there), the queries of the chunks and the fp32
    reference on the dequantized cache.

    Magnitudes: K rows are 0.5 x randn x factor, V rows 0.25 x randn x factor (|v| <= ~8).  The bf16
    kernel rounds P to bf16 (relative 2^-9, std 2^-9 / sqrt(3) = 0.0011) against an unrounded row sum,
    so an output is off by about 0.0011 x sqrt(sum p^2 v^2) <= 0.0011 x max |v| < 0.01 before its own
    bf16 rounding (relative, inside rtol): within atol = 2e-2 of test_attention_fa_prefill."""
    g = torch.Generator(device=DEV).manual_seed(17 + nh)
    ctxs = [p + n for p, n in zip(prefix, ntoks)]
    S = len(ctxs)
    maxp = max(math.ceil(c / PS) for c in ctxs) + 1
    P = S * maxp + 3
    rnd = lambda *s: torch.randn(*s, device=DEV, generator=g)  # noqa: E731
    fac = lambda: torch.exp2(torch.rand(P, nkv, PS, 1, device=DEV, generator=g) * 6 - 3)  # noqa: E731
    kf = ops.KVF8.from_dense(bf(0.5 * rnd(P, nkv, PS, D) * fac()))
    vf = ops.KVF8.from_dense(bf(0.25 * rnd(P, nkv, PS, D) * fac()))
    bt = torch.randperm(P, device=DEV, generator=g)[: S * maxp].view(S, maxp).to(torch.int32)
    for c in (kf, vf):  # one scale per tile, or a neighbouring row's scale, cannot pass on these
        assert c.scales[int(bt[0, 0]), 0].unique().numel() >= 4
    for i, c in enumerate(ctxs):
        pg = int(bt[i, (c - 1) // PS])
        for t in (kf.codes, kf.scales, vf.codes, vf.scales):
            t[pg, :, (c - 1) % PS + 1:] = 0xFF
    kd, vd = kf.dequant(), vf.dequant()
    assert bool(kd.isnan().any()) and bool(vd.isnan().any())
    q_seq = torch.cat([torch.full((n,), i, dtype=torch.int32) for i, n in enumerate(ntoks)]).to(DEV)
    q_ctx = torch.cat([torch.arange(p + 1, p + n + 1, dtype=torch.int32) for p, n in zip(prefix, ntoks)]).to(DEV)
    q = bf(rnd(q_seq.numel(), (nh + 2 * nkv) * D))  # strided q view like the executor's qkv
    o_ref = ref.paged_attention(q.float(), torch.nan_to_num(kd.float()), torch.nan_to_num(vd.float()), bt, q_seq,
                                q_ctx, nh, nkv, 1 / math.sqrt(D)).float()
    return q, kf, vf, kd, vd, bt, q_seq, q_ctx, o_ref


@pytest.mark.parametrize("nh,nkv", [(4, 4), (8, 4), (16, 4), (32, 4)])
@pytest.mark.parametrize("waves", [4, 8])
@pytest.mark.parametrize("parts,pair", [(None, False), (1, False), (3, False), (1, True)])
@pytest.mark.parametrize("ntoks,prefix", PROMPTS)
def test_attention_fa_f8_equals_bf16_kernel_on_dequantized_cache(nh, nkv, waves, parts, pair, ntoks, prefix):
    q, kf, vf, kd, vd, bt, q_seq, q_ctx, o_ref = _eq_case(nh, nkv, ntoks, prefix)
    fb = torch.from_numpy(ops.fa_blocks(ntoks, nh // nkv, waves)).to(DEV)
    assert int(fb[1].sum()) == q.shape[0]
    kw = dict(waves=waves, num_parts=parts, pair=pair)
    scale = 1 / math.sqrt(D)
    want = ops.attention_fa(q, kd, vd, bt, q_seq, q_ctx, fb, nh, nkv, scale, **kw)
    out = ops.attention_fa_f8(q, kf, vf, bt, q_seq, q_ctx, fb, nh, nkv, scale, **kw)
    assert torch.isfinite(out.float()).all()
    assert torch.equal(out, want)
    torch.testing.assert_close(want.float(), o_ref, atol=2e-2, rtol=2e-2)
    torch.testing.assert_close(out.float(), o_ref, atol=2e-2, rtol=2e-2)


# ---------------------------------------------------------------------------------------- probes
@functools.lru_cache(maxsize=None)
def _prefill(nh, nkv, ntoks, prefix):
    """The FA row selection of test_attention_probe_gpu.py: wave (32 rows), workgroup block (4 / 8
    waves) and 64-token step boundaries first."""
    tpw = 32 // (nh // nkv)
    rows = [0, 1]
    for m in (4, 8, 1, 2):
        rows += [m * tpw - 1, m * tpw]
    for n, pre in zip(ntoks, prefix):
        rows += [j for j in range(n) if (pre + j + 1) % 64 in (0, 1)]
    case = ap.prefill_case(nh, nkv, D, list(ntoks), list(prefix), row_idx=tuple(rows))
    return case, case.f8(DEV)


@pytest.mark.parametrize("nh,nkv", [(32, 8), (8, 4), (32, 32)])
@pytest.mark.parametrize("ntoks,prefix", [((130,), (0,)), ((129, 256), (0, 63)), ((300,), (64,))])
@pytest.mark.parametrize("waves,parts,pair", [(4, 1, False), (8, 1, False), (4, None, False), (8, None, False),
                                             (4, 3, False), (8, 3, False), (4, 1, True), (8, 1, True)])
def test_attention_fa_f8_probes(nh, nkv, ntoks, prefix, waves, parts, pair):
    """The cases of test_attention_fa_probes on the fp8 form of their caches (exact: ``Case.f8``
    asserts it), the poison as 0xFF codes and scales; the launch leaves the caches as they were."""
    case, (kc, vc) = _prefill(nh, nkv, ntoks, prefix)
    a = case.to(DEV)
    fb = torch.from_numpy(ops.fa_blocks(ntoks, nh // nkv, waves)).to(DEV)
    before = [t.clone() for t in (kc.codes, kc.scales, vc.codes, vc.scales)]
    out = ops.attention_fa_f8(a["q"], kc, vc, a["block_tables"], a["q_seq"], a["q_ctx"], fb, nh, nkv, case.scale,
                              waves=waves, num_parts=parts, pair=pair)
    _note("attention_fa_f8", ap.compare(out, case, f"attention_fa_f8 waves={waves} parts={parts} pair={pair}"))
    for t, t0 in zip((kc.codes, kc.scales, vc.codes, vc.scales), before):
        assert torch.equal(t, t0)


# ------------------------------------------------------------------------------------- refusals
def test_the_fa_f8_binding_refuses_what_the_kernel_does_not_cover():
    nh, nkv = 8, 4
    q, kf, vf, kd, vd, bt, q_seq, q_ctx, _ = _eq_case(nh, nkv, *PROMPTS[1])
    T = q.shape[0]
    fb = torch.from_numpy(ops.fa_blocks(PROMPTS[1][0], nh // nkv, 4)).to(DEV)
    out = torch.empty(T, nh * D, dtype=torch.bfloat16, device=DEV)
    ws = ops.attention_workspace(T, nh, D, 1, DEV)

    def call(k, v, ks, vs, fb_=fb, waves=4, q_=q, out_=out):
        torch.ops.mpamd.attention_fa(q_, k, v, bt, q_seq, q_ctx, fb_, out_, ws, nh, nkv, 1.0, 384, 1, waves, 0,
                                     k_scale=ks, v_scale=vs)

    call(kf.codes, vf.codes, kf.scales, vf.scales)  # the accepted form
    with pytest.raises(RuntimeError, match="uint8"):  # bf16 caches
        call(kd, vd, kf.scales, vf.scales)
    half = kf.scales[:, :, :32].contiguous()
    with pytest.raises(RuntimeError, match="scales"):  # scales of another page size
        call(kf.codes, vf.codes, half, half)
    k64 = ops.KVF8.from_dense(bf(torch.randn(4, nkv, PS, 64, device=DEV)))
    with pytest.raises(RuntimeError, match="head_dim 128"):
        call(k64.codes, k64.codes, k64.scales, k64.scales, q_=q[:, : (nh + 2 * nkv) * 64],
             out_=torch.empty(T, nh * 64, dtype=torch.bfloat16, device=DEV))
    with pytest.raises(RuntimeError, match="waves"):
        call(kf.codes, vf.codes, kf.scales, vf.scales, waves=5)
    with pytest.raises(RuntimeError, match="fablocks"):
        call(kf.codes, vf.codes, kf.scales, vf.scales, fb_=fb.cpu())
    torch.cuda.synchronize()
    # the op itself: bf16 caches are a TypeError, and the bf16 op still refuses a KVF8
    with pytest.raises(TypeError):
        ops.attention_fa_f8(q, kd, vd, bt, q_seq, q_ctx, fb, nh, nkv, 1.0)
    with pytest.raises(NotImplementedError, match="fp8 KV"):
        ops.attention_fa(q, kf, vf, bt, q_seq, q_ctx, fb, nh, nkv, 1.0)


# ----------------------------------------------------------------------------------------- executor
def _gqa4():
    return dataclasses.replace(resolve_model("small-llama"), num_key_value_heads=1, name="small-llama-gqa4")


def _fake_quant_hook(k, v):
    return ops.fake_quant_kv_fp8(k), ops.fake_quant_kv_fp8(v)


def _lens(B, long_at=3):
    lens = [5 + (7 * i) % 23 for i in range(B)]
    lens[long_at] = 70  # crosses a 64-token page
    return lens


def _count_calls(monkeypatch):
    """Wrap (not replace) the MFMA / FA2 attention ops: name -> calls."""
    calls = {}
    for name in ("attention_mfma", "attention_mfma_rope", "attention_fa", "attention_fa_f8", "attention_mfma_f8",
                 "attention_mfma_rope_f8"):
        real = getattr(ops, name)

        def wrapped(*a, _n=name, _real=real, **k):
            calls[_n] = calls.get(_n, 0) + 1
            return _real(*a, **k)

        monkeypatch.setattr(ops, name, wrapped)
    return calls


def _run(ex, cfg, calls, B=17, steps=3, chunked=False):
    """Prefill (whole, or 3 tokens of every prompt and then the rest) + ``steps`` decode steps ->
    (logits per step, sequences, ops.attention_fa_f8 calls of the last prefill step)."""
    g = torch.Generator().manual_seed(11)
    seqs = [torch.randint(0, cfg.vocab_size, (n,), generator=g).to(DEV) for n in _lens(B)]
    assert sum(len(s) for s in seqs) == 322
    names = [f"s{i}" for i in range(B)]
    if chunked:
        ex.forward([(n, 3) for n in names], torch.cat([s[:3] for s in seqs]))
        n0 = calls.get("attention_fa_f8", 0)
        lg = ex.forward([(n, len(s) - 3) for n, s in zip(names, seqs)], torch.cat([s[3:] for s in seqs]))
    else:
        n0 = calls.get("attention_fa_f8", 0)
        lg = ex.forward([(n, len(s)) for n, s in zip(names, seqs)], torch.cat(seqs))
    n_fa = calls.get("attention_fa_f8", 0) - n0
    outs = [lg.float().clone()]
    for _ in range(steps):
        nxt = torch.argmax(lg.float(), -1)
        seqs = [torch.cat([s, nxt[i:i + 1]]) for i, s in enumerate(seqs)]
        lg = ex.forward([(n, 1) for n in names], nxt)
        outs.append(lg.float().clone())
    torch.cuda.synchronize()
    return outs, seqs, n_fa


def _check_oracle(wd, outs, seqs, rows):
    for i in rows:
        want = reference_forward([wd], seqs[i], kv_hook=_fake_quant_hook)[-1].float()
        cos = torch.nn.functional.cosine_similarity(outs[-1][i], want, dim=0)
        assert float(cos) > 0.99, (i, float(cos))


def _executor_case(cfg, monkeypatch, chunked):
    """hipGraphs off and on: the prefill step runs ops.attention_fa_f8 in every layer and never
    ops.attention_fa, both runs agree bit for bit, the last logits track the fake-quantized oracle."""
    calls = _count_calls(monkeypatch)
    w = random_stage_weights(cfg, 0, cfg.num_hidden_layers, has_embed=True, has_head=True, device=DEV, seed=3)
    outs = {}
    for g in (False, True):
        ex = StageExecutor(cfg, w, DEV, kv_cache_bytes=64 << 20, max_sessions=32, max_seq_len=128, use_graphs=g,
                           kv_cache_dtype="fp8")
        assert ex.cache.is_fp8 and ex.prefill_fa_f8
        outs[g] = _run(ex, cfg, calls, chunked=chunked)
        assert ex.last_graphed == g
        assert outs[g][2] >= cfg.num_hidden_layers, calls
    for a, b in zip(outs[False][0], outs[True][0]):
        assert torch.equal(a, b)
    assert calls.get("attention_fa", 0) == 0, calls
    _check_oracle(w, outs[True][0], outs[True][1], rows=(0, 3, 16))
    return calls


@pytest.mark.parametrize("chunked", [False, True])
def test_executor_fp8_kv_prefill_runs_the_fa_f8_kernel(chunked, monkeypatch):
    """small-llama (MHA 4 / 4 / 128), 17 ragged sessions (one past a page, 322 prompt tokens: off the
    packed path), prefill + 3 decode steps; chunked: the second chunk attends to the first one's pages."""
    monkeypatch.delenv("MPAMD_KV_FP8_FA", raising=False)
    cfg = resolve_model("small-llama")
    assert (cfg.num_attention_heads, cfg.num_key_value_heads, cfg.head_dim) == (4, 4, 128)
    _executor_case(cfg, monkeypatch, chunked)


@pytest.mark.parametrize("chunked", [False, True])
def test_executor_fp8_kv_gqa4_prefill_fa_f8_and_decode_mfma_f8(chunked, monkeypatch):
    monkeypatch.delenv("MPAMD_KV_FP8_FA", raising=False)
    monkeypatch.delenv("MPAMD_KV_FP8_MFMA", raising=False)
    cfg = _gqa4()
    assert cfg.num_attention_heads // cfg.num_key_value_heads == 4 and cfg.head_dim == 128
    calls = _executor_case(cfg, monkeypatch, chunked)
    assert calls.get("attention_mfma_rope_f8", 0) >= 1, calls


def test_executor_fp8_kv_fa_switch_restores_the_flash_decoding_kernel(monkeypatch):
    monkeypatch.setenv("MPAMD_KV_FP8_FA", "0")
    calls = _count_calls(monkeypatch)
    cfg = resolve_model("small-llama")
    w = random_stage_weights(cfg, 0, cfg.num_hidden_layers, has_embed=True, has_head=True, device=DEV, seed=3)
    ex = StageExecutor(cfg, w, DEV, kv_cache_bytes=64 << 20, max_sessions=32, max_seq_len=128, kv_cache_dtype="fp8")
    assert ex.cache.is_fp8 and not ex.prefill_fa_f8
    outs, seqs, n_fa = _run(ex, cfg, calls)
    assert n_fa == 0 and calls.get("attention_fa_f8", 0) == 0, calls
    _check_oracle(w, outs, seqs, rows=(0, 3, 16))
