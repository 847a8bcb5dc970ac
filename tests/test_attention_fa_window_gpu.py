"""The FA2 prefill kernel's sliding-window form on the GPU (csrc/attention_fa.hip WIN form,
ops.attention_fa_window / attention_fa_window_f8): the prefill window probes
(tests/attn_window_prefill_probe.py) for WHICH keys it reads, bit equality of the fp8 form with the bf16
form on the dequantized cache and of W >= max_ctx with the unwindowed kernel, random inputs against the
windowed reference, and the executor's route for row-major prefill steps past the window.

Probes: W in 1 / 33 / 64 / 100, one launch of a 130-token prompt, a 70-token chunk at prefix 200, a
40-token chunk at prefix 0 and (MHA) a 200-token chunk at prefix 60; NaN below every sequence's first
``lo`` and all-NaN pages below that; the lower trap ``g (K[lo] + K[lo - 1])`` on rows whose ``lo - 1`` is
another row's key.  The comparator allows 2^-6, derived in attn_probe.py.

Largest |out - closed form| measured on an MI355X over all probes of all launches, next to the bound
2^-6 = 0.015625 (``pytest -s`` prints them again as WINDOW_FA_PROBE_DEV lines):
    attention_fa_window      0.008328
    attention_fa_window_f8   0.008328
(the unwindowed FA2 kernel's own figure: the bf16 rounding of the output and of P in the numerator
against an unrounded row sum l)."""
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
from tests import attn_window_prefill_probe as pp

pytestmark = pytest.mark.gpu
DEV = "cuda"
D = 128
SHAPES = [(4, 4), (4, 2), (8, 2), (8, 1)]  # HB 1 / 2 / 4 / 8

_SEEN = {}


@pytest.fixture(scope="module", autouse=True)
def _native():
    assert ops.load_library(), "HIP kernel library must load on the GPU box"
    yield
    for k, v in sorted(_SEEN.items()):
        print(f"\nWINDOW_FA_PROBE_DEV {k} {v:.6f}", end="")


def _note(kernel, dev):
    _SEEN[kernel] = max(_SEEN.get(kernel, 0.0), dev)


@functools.lru_cache(maxsize=None)
def _case(nh, nkv, W):
    """(case, its tensors on the GPU, its fp8 caches, the bf16 caches of their dequantized values)."""
    case = pp.prefill_window_case(nh, nkv, W)
    kf, vf = case.f8(DEV)
    return case, case.to(DEV), (kf, vf), (kf.dequant(), vf.dequant())


def _meta(a):
    return a["block_tables"], a["q_seq"], a["q_ctx"]


def _fb(case, waves):
    return torch.from_numpy(ops.fa_blocks(pp.ntoks(case), case.nh // case.nkv, waves)).to(DEV)


# ------------------------------------------------------------------------------------ probes
@pytest.mark.parametrize("nh,nkv", SHAPES)
@pytest.mark.parametrize("W", pp.WINDOWS)
@pytest.mark.parametrize("waves", [4, 8])
def test_attention_fa_window_probes(nh, nkv, W, waves):
    """Both cache kinds through the wrapper's own partition, explicit slices of 64 / 128 / 256 tokens with
    two empty trailing ones, and one part with the pairing off and on; the fp8 form equals the bf16 form
    on the dequantized cache bit for bit in every launch."""
    case, a, (kf, vf), (kd, vd) = _case(nh, nkv, W)
    fb = _fb(case, waves)
    assert int(fb[1].sum()) == case.T and int(fb[1].max()) <= pp.block_tokens(nh, nkv, waves)
    mc = int(case.q_ctx.max())
    launches = [dict()] + [dict(part_size=ps, num_parts=np_, max_ctx=mc) for ps, np_ in pp.partitions(case, W, waves)]
    launches += [dict(num_parts=1, pair=False), dict(num_parts=1, pair=True)]
    for kw in launches:
        what = f"W={W} waves={waves} {kw}"
        out = ops.attention_fa_window(a["q"], a["k_cache"], a["v_cache"], *_meta(a), fb, nh, nkv, case.scale, W,
                                      waves=waves, **kw)
        _note("attention_fa_window", ap.compare(out, case, f"attention_fa_window {what}"))
        out8 = ops.attention_fa_window_f8(a["q"], kf, vf, *_meta(a), fb, nh, nkv, case.scale, W, waves=waves, **kw)
        _note("attention_fa_window_f8", ap.compare(out8, case, f"attention_fa_window_f8 {what}"))
        outd = ops.attention_fa_window(a["q"], kd, vd, *_meta(a), fb, nh, nkv, case.scale, W, waves=waves, **kw)
        assert torch.equal(out8, outd), what
    assert torch.equal(a["q"].cpu(), case.q)


def test_the_window_binding_refuses_what_it_does_not_cover():
    nh, nkv, W = 8, 2, 33
    case, a, (kf, vf), _ = _case(nh, nkv, W)
    fb = _fb(case, 4)
    out = torch.empty(case.T, nh * D, dtype=torch.bfloat16, device=DEV)
    ws = ops.attention_workspace(case.T, nh, D, 1, DEV)
    args = (a["q"], a["k_cache"], a["v_cache"], *_meta(a), fb, out, ws, nh, nkv, case.scale, 320, 1, 4, 0)
    torch.ops.mpamd.attention_fa_window(*args, W)  # the accepted form
    ap.compare(out, case, "mpamd::attention_fa_window")
    for bad in (0, -1):
        with pytest.raises(RuntimeError, match="window"):
            torch.ops.mpamd.attention_fa_window(*args, bad)
    with pytest.raises(RuntimeError, match="waves"):
        torch.ops.mpamd.attention_fa_window(*args[:-2], 5, 0, W)
    with pytest.raises(RuntimeError, match="uint8"):
        torch.ops.mpamd.attention_fa_window(*args, W, k_scale=kf.scales, v_scale=vf.scales)
    with pytest.raises(ValueError, match="cover"):
        ops.attention_fa_window(a["q"], a["k_cache"], a["v_cache"], *_meta(a), fb, nh, nkv, case.scale, W, waves=4,
                                part_size=64, num_parts=1, max_ctx=int(case.q_ctx.max()))
    with pytest.raises(ValueError, match="window"):
        ops.attention_fa_window(a["q"], a["k_cache"], a["v_cache"], *_meta(a), fb, nh, nkv, case.scale, 0)
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------ unwindowed
@pytest.mark.parametrize("nh,nkv", SHAPES)
@pytest.mark.parametrize("f8", [False, True])
def test_window_at_or_above_the_context_is_the_unwindowed_kernel(nh, nkv, f8):
    """W >= max_ctx: base = 0, every lo = 0 - the same slices and the same arithmetic as ops.attention_fa
    launched with the same waves, num_parts and pair."""
    ntoks, prefix = (129, 256, 40), (0, 63, 200)
    case = ap.prefill_case(nh, nkv, D, list(ntoks), list(prefix))
    a = case.to(DEV)
    kc, vc = case.f8(DEV) if f8 else (a["k_cache"], a["v_cache"])
    plain = ops.attention_fa_f8 if f8 else ops.attention_fa
    win = ops.attention_fa_window_f8 if f8 else ops.attention_fa_window
    mc = int(case.q_ctx.max())
    for waves in (4, 8):
        fb = torch.from_numpy(ops.fa_blocks(ntoks, nh // nkv, waves)).to(DEV)
        for W in (mc, 100000):
            for kw in (dict(), dict(num_parts=1, pair=False), dict(num_parts=1, pair=True), dict(num_parts=3)):
                o0 = plain(a["q"], kc, vc, *_meta(a), fb, nh, nkv, case.scale, waves=waves, **kw)
                o1 = win(a["q"], kc, vc, *_meta(a), fb, nh, nkv, case.scale, W, waves=waves, **kw)
                assert torch.equal(o0, o1), (W, waves, kw)
                ap.compare(o1, case, f"W={W} >= max_ctx")


# ------------------------------------------------------------------------------------ random inputs
def _random_prefill(nh, nkv, ntoks, prefix, seed=0):
    """randn q and caches for chunks of ``ntoks`` tokens at ``prefix``: bf16 and fp8 caches of the same
    values (rows of different magnitudes, so the e8m0 scales differ inside a tile), 0xFF / NaN past
    every sequence's last token to the end of its page."""
    g = torch.Generator(device=DEV).manual_seed(seed)
    ctxs = [p + n for p, n in zip(prefix, ntoks)]
    npg = [math.ceil(c / 64) for c in ctxs]
    P = sum(npg) + 2
    rnd = lambda *s: torch.randn(*s, device=DEV, generator=g)  # noqa: E731
    fac = lambda: torch.exp2(torch.rand(P, nkv, 64, 1, device=DEV, generator=g) * 4 - 2)  # noqa: E731
    kf = ops.KVF8.from_dense((0.5 * rnd(P, nkv, 64, D) * fac()).to(torch.bfloat16))
    vf = ops.KVF8.from_dense((0.25 * rnd(P, nkv, 64, D) * fac()).to(torch.bfloat16))
    perm = torch.randperm(P, device=DEV, generator=g).tolist()
    bt = torch.full((len(ctxs), max(npg)), perm[-1], dtype=torch.int32)
    used = 0
    for i, n in enumerate(npg):
        bt[i, :n] = torch.tensor(perm[used:used + n], dtype=torch.int32)
        used += n
        if ctxs[i] % 64:
            for t in (kf.codes, kf.scales, vf.codes, vf.scales):
                t[int(bt[i, n - 1]), :, ctxs[i] % 64:] = 0xFF
    q_seq = torch.cat([torch.full((n,), i, dtype=torch.int32) for i, n in enumerate(ntoks)])
    q_ctx = torch.cat([torch.arange(p + 1, p + n + 1, dtype=torch.int32) for p, n in zip(prefix, ntoks)])
    q = rnd(q_seq.numel(), (nh + 2 * nkv) * D).to(torch.bfloat16)  # q strided inside a qkv row
    return q, kf, vf, bt.to(DEV), q_seq, q_ctx


@pytest.mark.parametrize("nh,nkv,W,ntoks,prefix", [
    (8, 2, 100, (130, 70, 40, 300), (0, 200, 0, 64)),  # contexts on both sides of W = 100
    (4, 4, 100, (130, 70, 40, 300), (0, 200, 0, 64)),
    (8, 2, 4096, (4200,), (0,)),                       # one 4200-token prompt across W = 4096
])
def test_window_fa_random_inputs_match_the_reference(nh, nkv, W, ntoks, prefix):
    """randn inputs against ``ops.reference.paged_attention(window=W)`` on the cache the kernel reads, under
    atol = rtol = 2e-2 (test_window_random_inputs_match_the_reference's bound); fp8 = bf16 bit for bit."""
    q, kf, vf, bt, q_seq, q_ctx = _random_prefill(nh, nkv, ntoks, prefix)
    kd, vd = kf.dequant(), vf.dequant()
    # the reference reads q_seq / q_ctx row by row: they stay on the host
    want = ref.paged_attention(q.float(), torch.nan_to_num(kd.float()), torch.nan_to_num(vd.float()), bt, q_seq, q_ctx,
                               nh, nkv, 1 / math.sqrt(D), window=W).float()
    for waves in (4, 8):
        fb = torch.from_numpy(ops.fa_blocks(ntoks, nh // nkv, waves)).to(DEV)
        for kw in (dict(), dict(num_parts=1)):
            out = ops.attention_fa_window(q, kd, vd, bt, q_seq.to(DEV), q_ctx.to(DEV), fb, nh, nkv, 1 / math.sqrt(D), W,
                                          waves=waves, **kw)
            out8 = ops.attention_fa_window_f8(q, kf, vf, bt, q_seq.to(DEV), q_ctx.to(DEV), fb, nh, nkv,
                                              1 / math.sqrt(D), W, waves=waves, **kw)
            assert torch.equal(out, out8), (waves, kw)
            torch.testing.assert_close(out.float(), want, atol=2e-2, rtol=2e-2)


# ------------------------------------------------------------------------------------ executor
# Steps of up to 256 rows may run the packed-activation path (attention output in the packed layout, which
# FA2 does not write); the stage decides per row count, and this model's steps are packed up to 128 rows.
# max_tokens_per_step = 160 splits the prompt into a 160-token chunk (row-major, contexts up to 160 > W)
# and a 90-token one (packed: it keeps the flash-decoding rows).  The test asserts that the chunked run
# has a row-major chunk past the window and a packed one, and does not assume it.
CHUNK = 160
PROMPT = 250


def _fake_quant_hook(k, v):
    return ops.fake_quant_kv_fp8(k), ops.fake_quant_kv_fp8(v)


def _cfg():
    cfg = dataclasses.replace(resolve_model("small-llama"), model_type="mistral", sliding_window=96,
                              name="small-mistral-w96")
    assert (cfg.num_attention_heads, cfg.num_key_value_heads, cfg.head_dim) == (4, 4, 128)
    return cfg


@functools.lru_cache(maxsize=None)
def _weights():
    cfg = _cfg()
    return random_stage_weights(cfg, 0, cfg.num_hidden_layers, has_embed=True, has_head=True, device=DEV,
                                dtype=torch.bfloat16, seed=4)


def _spy(monkeypatch, ex):
    """Record every ``_attend`` call (prefill?, packed, max_ctx) and which attention op it ran."""
    log = []
    for name in ("attention_fa_window", "attention_fa_window_f8", "attention_fa", "attention_fa_f8", "paged_attention",
                 "attention_mfma", "attention_mfma_f8"):
        real = getattr(ops, name)

        def wrapped(*a, _n=name, _real=real, **k):
            if log and log[-1]["op"] is None:
                log[-1]["op"] = _n
            return _real(*a, **k)

        monkeypatch.setattr(ops, name, wrapped)
    real_attend = ex._attend

    def attend(st, qkv, kc, vc, out, packed):
        log.append(dict(prefill=st.qblocks is not None, packed=bool(packed), max_ctx=int(st.max_ctx), op=None,
                        fb=st.fablocks is not None))
        return real_attend(st, qkv, kc, vc, out, packed)

    monkeypatch.setattr(ex, "_attend", attend)
    return log


@pytest.mark.parametrize("kv", ["bf16", "fp8"])
@pytest.mark.parametrize("switch", ["1", "0"])
def test_executor_prefill_past_the_window_runs_the_windowed_fa_kernel(kv, switch, monkeypatch):
    """A 250-token prompt in one step and in chunks of CHUNK tokens, W = 96: logits against the windowed
    fp32 oracle, held pages within ceil(W / 64) + 1, and the route: every row-major prefill step past the
    window on the windowed FA2 op, no other step on it (packed chunks, decode, steps inside the window), none
    at all with MPAMD_WINDOW_FA=0."""
    monkeypatch.setenv("MPAMD_WINDOW_FA", switch)
    monkeypatch.delenv("MPAMD_KV_FP8_FA", raising=False)
    cfg, w = _cfg(), _weights()
    W = cfg.sliding_window
    new_op = "attention_fa_window_f8" if kv == "fp8" else "attention_fa_window"
    ids = torch.randint(0, cfg.vocab_size, (PROMPT,), generator=torch.Generator().manual_seed(5))
    want = reference_forward([w], ids.to(DEV), kv_hook=_fake_quant_hook if kv == "fp8" else None, window=W)[-1]
    for kw in ({}, dict(max_tokens_per_step=CHUNK)):
        ex = StageExecutor(cfg, w, DEV, kv_cache_bytes=64 << 20, max_sessions=4, use_graphs=False, kv_cache_dtype=kv,
                           sliding_window="attend", **kw)
        assert ex.window == W and ex.window_fa == (switch == "1") and ex._attn_fa
        assert kv == "bf16" or ex.prefill_fa_f8
        with monkeypatch.context() as mp:
            log = _spy(mp, ex)
            lg = ex.forward([("s", PROMPT)], ids.to(DEV))
            nxt = torch.argmax(lg.float(), -1)
            ex.forward([("s", 1)], nxt)  # a decode step past the window: never the prefill op
        torch.testing.assert_close(lg[0].float(), want, atol=0.06, rtol=0.05)
        assert len(ex.sessions.get("s").pages) <= math.ceil(W / 64) + 1
        assert all(c["op"] is not None for c in log)
        past = [c for c in log if c["prefill"] and c["fb"] and not c["packed"] and c["max_ctx"] > W]
        rest = [c for c in log if c not in past]
        if kw:  # the chunk size was chosen for this
            assert past, f"no row-major prefill chunk past the window at max_tokens_per_step={CHUNK}: {log}"
            assert any(c["prefill"] and c["packed"] and c["max_ctx"] > W for c in log)
        print(f"\nWINDOW_FA_ROUTE kv={kv} switch={switch} {kw}: " +
              ", ".join(sorted({f"{c['op']}(packed={c['packed']}, past={c['max_ctx'] > W})" for c in log})), end="")
        if switch == "1":
            assert all(c["op"] == new_op for c in past), past
        else:
            assert all(c["op"] == "paged_attention" for c in past), past
        assert all(c["op"] not in ("attention_fa_window", "attention_fa_window_f8") for c in rest), rest
        # a row-major prefill step inside the window (3 x 50 tokens): the unwindowed FA2 kernel, as before
        with monkeypatch.context() as mp:
            log = _spy(mp, ex)
            ex.forward([(n, 50) for n in "abc"], ids[:150].to(DEV))
        assert log and all(c["prefill"] and not c["packed"] and c["max_ctx"] == 50 for c in log), log
        assert all(c["op"] == ("attention_fa_f8" if kv == "fp8" else "attention_fa") for c in log), log
