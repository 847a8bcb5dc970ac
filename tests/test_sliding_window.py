"""Sliding-window attention on the CPU path: the reference op, the window probes, rolling KV pages in
the session table, a stage run against the windowed fp32 oracle, HF Mistral parity and the CLI switch.

Semantics (HF Mistral, eager and sdpa): with window W the query at position i sees keys j with
0 <= i - j < W - W keys, its own included.  A query row of context ``ctx`` (its own token included)
sees cache positions [max(0, ctx - W), ctx)."""
import dataclasses
import math

import pytest
import torch

from src.models.config import resolve_model
from src.models.reference_model import reference_forward
from src.models.weights import random_stage_weights
from src.ops import reference as ref
from src.runtime.executor import StageExecutor
from src.runtime.kv_cache import PagedKVCache
from src.runtime.kv_layout import export_session_kv
from src.runtime.session import SessionManager
from tests import attn_probe as ap
from tests import attn_window_probe as wp

PAGE = 64


# ------------------------------------------------------------------------------------ the reference op
def _paged(nkv, D, ctxs, gen, dtype=torch.float64):
    """Random caches with one sequence per context, pages in shuffled order."""
    npg = [math.ceil(c / PAGE) for c in ctxs]
    P = sum(npg) + 1
    perm = torch.randperm(P, generator=gen).tolist()
    kc = torch.randn(P, nkv, PAGE, D, generator=gen, dtype=dtype)
    vc = torch.randn(P, nkv, PAGE, D, generator=gen, dtype=dtype)
    bt = torch.full((len(ctxs), max(npg)), -1, dtype=torch.int32)
    used = 0
    for i, n in enumerate(npg):
        bt[i, :n] = torch.tensor(perm[used:used + n], dtype=torch.int32)
        used += n
    return kc, vc, bt


@pytest.mark.parametrize("W", [1, 5, 64, 100])
def test_reference_window_equals_dense_masked_softmax(W):
    nh, nkv, D = 4, 2, 16
    g = torch.Generator().manual_seed(W)
    ctxs = sorted({1, max(1, W - 1), W, W + 1, W + 63, W + 64, 2 * W + 70})  # below, at and above W
    kc, vc, bt = _paged(nkv, D, ctxs, g, torch.float32)
    q = torch.randn(len(ctxs), nh * D, generator=g)
    q_seq = torch.arange(len(ctxs), dtype=torch.int32)
    q_ctx = torch.tensor(ctxs, dtype=torch.int32)
    out = ref.paged_attention(q, kc, vc, bt, q_seq, q_ctx, nh, nkv, 0.25, window=W).view(len(ctxs), nh, D)
    full = ref.paged_attention(q, kc, vc, bt, q_seq, q_ctx, nh, nkv, 0.25).view(len(ctxs), nh, D)
    for t, n in enumerate(ctxs):
        pages = bt[t, : math.ceil(n / PAGE)].long()
        k = kc[pages].permute(1, 0, 2, 3).reshape(nkv, -1, D)[:, :n].repeat_interleave(nh // nkv, 0).double()
        v = vc[pages].permute(1, 0, 2, 3).reshape(nkv, -1, D)[:, :n].repeat_interleave(nh // nkv, 0).double()
        s = torch.einsum("hd,hnd->hn", q[t].view(nh, D).double(), k) * 0.25
        j = torch.arange(n)
        s = s.masked_fill(~((n - 1 - j >= 0) & (n - 1 - j < W)), float("-inf"))
        want = torch.einsum("hn,hnd->hd", torch.softmax(s, -1), v)
        # the reference computes in fp32: sums over n <= 270 keys of O(1) terms, n * 2^-24 < 2e-5
        torch.testing.assert_close(out[t].double(), want, atol=2e-5, rtol=2e-5)
        if n <= W:
            assert torch.equal(out[t], full[t])
    with pytest.raises(ValueError, match="window"):
        ref.paged_attention(q, kc, vc, bt, q_seq, q_ctx, nh, nkv, 0.25, window=-1)


def test_reference_window_never_looks_up_released_pages():
    """Block-table entries of pages wholly below the window may be -1 (released)."""
    nh, nkv, D, W = 2, 1, 16, 70
    g = torch.Generator().manual_seed(0)
    kc, vc, bt = _paged(nkv, D, [300], g, torch.float32)
    q = torch.randn(1, nh * D, generator=g)
    args = (torch.zeros(1, dtype=torch.int32), torch.tensor([300], dtype=torch.int32), nh, nkv, 0.25)
    want = ref.paged_attention(q, kc, vc, bt, *args, window=W)
    bt2 = bt.clone()
    bt2[0, : (300 - W) // PAGE] = -1
    kc2, vc2 = kc.clone(), vc.clone()
    kc2[bt[0, : (300 - W) // PAGE].long()] = float("nan")
    assert torch.equal(ref.paged_attention(q, kc2, vc2, bt2, *args, window=W), want)


@pytest.mark.parametrize("mfma", [False, True])
@pytest.mark.parametrize("W", wp.WINDOWS)
def test_window_probes_accept_the_reference_and_reject_a_wider_window(W, mfma):
    """The probe cases are consistent (the reference passes at 2^-6, on the bf16 and the fp8 cache) and
    can tell: one key too many below ``lo`` (window W + 1, or none) gives a non-finite row."""
    nh, nkv, D = (16, 4, 64) if mfma else (8, 2, 64)
    case = wp.window_case(nh, nkv, D, W, mfma=mfma)
    a = (case.q.float(), case.k_cache.float(), case.v_cache.float(), case.block_tables, case.q_seq, case.q_ctx)
    ap.compare(ref.paged_attention(*a, nh, nkv, case.scale, window=W), case, f"reference W={W}")
    kf, vf = case.f8()
    ap.compare(ref.paged_attention_f8(a[0], kf, vf, *a[3:], nh, nkv, case.scale, window=W), case, f"reference f8 W={W}")
    for wide in (W + 1, 0):
        with pytest.raises(AssertionError, match="non-finite"):
            ap.compare(ref.paged_attention(*a, nh, nkv, case.scale, window=wide), case)
    # every page wholly below a row's window is named by the all-NaN page, and lo itself is a probed key
    for si, seq in enumerate(case.seqs):
        n = int(case.q_ctx[seq.rows[0]])
        lo = wp.lo_of(n, W)
        assert all(bool(case.poison[int(case.block_tables[si, j])].all()) for j in range(lo // PAGE))
        assert any(lo in p.keys for t in seq.rows for p in case.probes[t])
        assert lo == 0 or seq.K[lo - 1].isnan().all()
    rc = wp.window_rope_case(nh, nkv, D, W, mfma=mfma)
    q = rc.q.float().clone()
    kc, vc = rc.k_cache.float().clone(), rc.v_cache.float().clone()
    ref.rope_kv_write(q, rc.positions, rc.cos, rc.sin, kc, vc, rc.slots, nh, nkv)
    ap.compare(ref.paged_attention(q, kc, vc, rc.block_tables, rc.q_seq, rc.q_ctx, nh, nkv, rc.scale, window=W), rc,
               f"reference rope W={W}")
    wp.check_cache_after(rc, kc.to(ap.BF), vc.to(ap.BF), False)


# ------------------------------------------------------------------------------------ rolling pages
def _manager(W, max_seq_len=1024, pages=64, sessions=4):
    cache = PagedKVCache(1, pages, 1, 8, PAGE, torch.float32, "cpu")
    return SessionManager(cache, sessions, max_seq_len, window=W), cache


def _step(sm, s, n):
    """What the executor does around a step of n tokens: reserve, (run), commit, release."""
    sm.reserve(s, s.length + n)
    s.length += n
    sm.release(s)


@pytest.mark.parametrize("W", [1, 5, 64, 100])
@pytest.mark.parametrize("chunk", [1, 50])
def test_held_pages_stay_within_the_window_bound(W, chunk):
    sm, cache = _manager(W)
    free0 = sm.free_pages
    s = sm.open("a")
    bound = math.ceil(W / PAGE) + 1
    total = 4 * W + 70
    while s.length < total:
        n = min(chunk, total - s.length)
        _step(sm, s, n)
        L = s.length
        assert len(s.pages) <= bound, (L, len(s.pages))
        first = max(0, L + 1 - W) // PAGE  # pages wholly below position L + 1 - W are gone
        assert s.first_page == first
        row = sm.table[s.row]
        assert (row[:first] == -1).all() and (row[first + len(s.pages):] == -1).all()
        assert row[first:first + len(s.pages)].tolist() == s.pages and all(p >= 0 for p in s.pages)
        assert sm.free_pages == free0 - len(s.pages)
    assert s.first_page > 0 or W >= total
    sm.close("a")
    assert sm.free_pages == free0 and (sm.table == -1).all()


def test_no_window_keeps_every_page():
    sm, _ = _manager(0)
    s = sm.open("a")
    for _ in range(300):
        _step(sm, s, 1)
    assert s.first_page == 0 and len(s.pages) == math.ceil(300 / PAGE)


def test_rewind_rule_and_lifecycle():
    W = 100
    sm, cache = _manager(W)
    free0 = sm.free_pages
    s = sm.open("a")
    for _ in range(6):
        _step(sm, s, 50)  # L = 300: pages below position 201 // 64 * 64 = 192 are released
    assert s.first_page == 3 and s.length == 300
    # a rewind to p is allowed exactly while position max(0, p + 1 - W) is still held
    for p in range(299, -1, -1):
        ok = max(0, p + 1 - W) // PAGE >= s.first_page
        assert ok == (p >= 291)
        if not ok:
            with pytest.raises(ValueError, match="window"):
                sm.rewind(s, p)
            assert s.length == 291
        else:
            sm.rewind(s, p)
            assert s.length == p
    _step(sm, s, 20)  # goes on from the rewound position with the pages it holds
    assert s.length == 311 and s.first_page == 3
    with pytest.raises(ValueError, match="rolled"):
        export_session_kv(cache, s)
    # rename keeps the rolled state; reset starts over from page 0; evict_expired returns everything
    s2 = sm.rename("a", "b")
    assert s2 is s and s2.first_page == 3 and sm.get("a") is None
    sm.reset("b")
    assert s.first_page == 0 and s.pages == [] and sm.free_pages == free0 and (sm.table == -1).all()
    _step(sm, s, 10)
    assert s.first_page == 0 and len(s.pages) == 1
    s.last_used -= 10 * sm.ttl
    assert sm.evict_expired() == 1 and sm.free_pages == free0


def test_fork_of_a_rolled_session_attends_identically():
    W, nh, nkv, D = 100, 1, 1, 8
    sm, cache = _manager(W)
    g = torch.Generator().manual_seed(0)
    cache.k[0].copy_(torch.randn(cache.k[0].shape, generator=g))
    cache.v[0].copy_(torch.randn(cache.v[0].shape, generator=g))
    s = sm.open("a")
    for _ in range(6):
        _step(sm, s, 50)
    free1 = sm.free_pages
    d = sm.fork("a", "b")
    assert d.first_page == s.first_page == 3 and len(d.pages) == len(s.pages) and d.length == 300
    assert sm.free_pages == free1 - len(s.pages) and not set(d.pages) & set(s.pages)  # only the held pages
    assert (sm.table[d.row][:3] == -1).all()
    q = torch.randn(1, nh * D, generator=g).repeat(2, 1)  # the same query on the source and on the fork
    kc, vc = cache.layer(0)
    out = ref.paged_attention(q, kc, vc, torch.from_numpy(sm.table.copy()),
                              torch.tensor([s.row, d.row], dtype=torch.int32),
                              torch.tensor([300, 300], dtype=torch.int32), nh, nkv, 0.3, window=W)
    assert torch.equal(out[0], out[1]) and bool(out[0].abs().sum() > 0)
    # reorder (beam search) forks through the same path
    sm.reorder(["a", "b"], [1, 0])
    assert sm.get("a").first_page == 3 and sm.get("b").first_page == 3
    sm.close("a")
    sm.close("b")
    assert sm.free_pages == cache.allocator.free_pages == 64


# ------------------------------------------------------------------------------------ a stage run
def _mistral_cfg():
    return dataclasses.replace(resolve_model("tiny-llama"), model_type="mistral", sliding_window=96)


@pytest.fixture(scope="module")
def stage():
    cfg = _mistral_cfg()
    w = random_stage_weights(cfg, 0, cfg.num_hidden_layers, has_embed=True, has_head=True, device="cpu",
                             dtype=torch.float32, seed=11)
    return cfg, w


@pytest.mark.parametrize("prompt,chunk", [(70, None), (250, 64)])
def test_stage_attends_past_the_window_like_the_windowed_oracle(stage, prompt, chunk):
    """Prefill (whole, or chunked under max_tokens_per_step=64), then decode to 300 tokens: the last
    token's logits equal the windowed fp32 oracle at every checked length; pages stay bounded."""
    cfg, w = stage
    W = cfg.sliding_window
    kw = dict(max_tokens_per_step=chunk) if chunk else {}
    ex = StageExecutor(cfg, w, "cpu", dtype=torch.float32, kv_cache_bytes=8 << 20, max_sessions=2,
                       sliding_window="attend", **kw)
    assert ex.max_seq_len == cfg.max_position_embeddings != W and ex.window == W and ex.sliding_window == "attend"
    ids = torch.randint(0, cfg.vocab_size, (prompt,), generator=torch.Generator().manual_seed(prompt))
    lg = ex.forward([("s", prompt)], ids)
    s = ex.sessions.get("s")
    bound = math.ceil(W / PAGE) + 1
    while True:
        L = ids.numel()
        assert s.length == L and len(s.pages) <= bound
        if L in (prompt, 95, 96, 97, 128, 129, 161, 200, 257, 300):
            torch.testing.assert_close(lg[0], reference_forward([w], ids, window=W)[-1], atol=1e-4, rtol=1e-4)
        if L == 300:
            break
        nxt = torch.argmax(lg, -1)
        ids = torch.cat([ids, nxt])
        lg = ex.forward([("s", 1)], nxt)
    assert s.first_page == (300 + 1 - W) // PAGE > 0
    # the unwindowed oracle is something else by now: the window is really applied
    assert not torch.allclose(lg[0], reference_forward([w], ids)[-1], atol=1e-4, rtol=1e-4)
    # a rewind inside the held pages replays; one below them names the window
    ex.forward([("s", 1)], ids[-1:], starts=[299])
    with pytest.raises(ValueError, match="window"):
        ex.forward([("s", 1)], ids[:1], starts=[100])


def test_default_mode_still_caps_and_unwindowed_models_ignore_the_switch(stage):
    cfg, w = stage
    ex = StageExecutor(cfg, w, "cpu", dtype=torch.float32, kv_cache_bytes=8 << 20, max_sessions=2)
    assert ex.max_seq_len == 96 and ex.window == 0 and ex.sliding_window == "cap" and ex.sessions.window == 0
    with pytest.raises(ValueError, match="sliding_window"):
        StageExecutor(cfg, w, "cpu", dtype=torch.float32, kv_cache_bytes=8 << 20, max_sessions=2, sliding_window="on")
    for name in ("tiny-llama", "tiny-gpt2"):
        c = resolve_model(name)
        wl = random_stage_weights(c, 0, 1, has_embed=True, has_head=False, device="cpu", dtype=torch.float32)
        e = StageExecutor(c, wl, "cpu", dtype=torch.float32, kv_cache_bytes=8 << 20, max_sessions=2,
                          sliding_window="attend")
        assert e.window == 0 and e.sliding_window is None and e.max_seq_len == c.max_position_embeddings


def test_op_wrappers_take_window_on_the_cpu_path():
    from src import ops

    nh, nkv, D, W = 4, 2, 16, 70
    g = torch.Generator().manual_seed(1)
    kc, vc, bt = _paged(nkv, D, [300, 50], g, torch.float32)
    q = torch.randn(2, nh * D, generator=g)
    q_seq = torch.arange(2, dtype=torch.int32)
    q_ctx = torch.tensor([300, 50], dtype=torch.int32)
    want = ref.paged_attention(q, kc, vc, bt, q_seq, q_ctx, nh, nkv, 0.25, window=W)
    assert torch.equal(ops.paged_attention(q, kc, vc, bt, q_seq, q_ctx, nh, nkv, 0.25, window=W), want)
    qb = torch.from_numpy(ops.query_blocks([1, 1], nh // nkv))
    assert torch.equal(ops.attention_mfma(q, kc, vc, bt, q_seq, q_ctx, qb, nh, nkv, 0.25, window=W), want)
    assert not torch.equal(ops.paged_attention(q, kc, vc, bt, q_seq, q_ctx, nh, nkv, 0.25), want)
    # explicit slices must cover the streamed span: min(max_ctx, W) / min(max_ctx, W + 31)
    ops._check_window_parts("paged_attention", W, 300, 64, 2)
    ops._check_window_parts("attention_mfma", W, 300, 128, 1, 31)
    ops._check_window_parts("paged_attention", W, 50, 64, 1)
    with pytest.raises(ValueError, match="cover"):
        ops._check_window_parts("paged_attention", W, 300, 64, 1)
    with pytest.raises(ValueError, match="cover"):
        ops._check_window_parts("attention_mfma", 100, 300, 128, 1, 31)
    assert ops._window_span(0, 300) == 300 and ops._window_span(W, 300) == W and ops._window_span(W, 300, 31) == W + 31


# ------------------------------------------------------------------------------------ HF parity
def test_hf_mistral_two_stage_attend_matches_transformers(tmp_path):
    """A tiny random ``MistralForCausalLM`` with sliding_window=16 through ``load_stage_model`` (two
    stages) with ``sliding_window="attend"``: a 40-token prompt and 8 greedy steps, each step's logits
    against HF's uncached forward of the whole sequence (tolerance of test_hf_parity.py's Llama check)."""
    tr = pytest.importorskip("transformers")
    from src.llama_partition import Stage0, StageLast, load_stage_model

    hcfg = tr.MistralConfig(vocab_size=256, hidden_size=128, intermediate_size=256, num_hidden_layers=3,
                            num_attention_heads=4, num_key_value_heads=2, max_position_embeddings=512,
                            sliding_window=16, tie_word_embeddings=False, rms_norm_eps=1e-5)
    torch.manual_seed(0)
    model = tr.MistralForCausalLM(hcfg).float().eval()
    with torch.no_grad():
        for n, p in model.named_parameters():
            if "norm" in n:
                p.uniform_(0.5, 1.5)
    model.save_pretrained(tmp_path)
    cfg = resolve_model(str(tmp_path))
    assert cfg.model_type == "mistral" and cfg.sliding_window == 16
    kw = dict(kv_cache_bytes=8 << 20, max_sessions=2, max_seq_len=128, sliding_window="attend")
    f0 = load_stage_model(str(tmp_path), "cpu", "stage0", end=1, dtype=torch.float32, **kw)
    f1 = load_stage_model(str(tmp_path), "cpu", "last", start=1, dtype=torch.float32, **kw)
    s0, s1 = Stage0(f0, 1), StageLast(f1, 1)
    assert s0.executor.window == 16 and s0.executor.max_seq_len == 128
    n = 40
    ids = torch.randint(0, 256, (1, n), generator=torch.Generator().manual_seed(3))
    with torch.no_grad():
        want = model(ids).logits[0, -1]
        h, p0 = s0(ids, torch.arange(n)[None], None, None)
        lg, p1 = s1(h, torch.arange(n)[None], None, None)
    torch.testing.assert_close(lg[0, -1], want, atol=2e-4, rtol=2e-4)
    seq = ids
    for _ in range(8):
        nxt = torch.argmax(lg[0, -1]).view(1, 1)
        seq = torch.cat([seq, nxt], 1)
        pos = torch.tensor([[seq.shape[1] - 1]])
        with torch.no_grad():
            want = model(seq).logits[0, -1]
            h, p0 = s0(nxt, pos, None, p0)
            lg, p1 = s1(h, pos, None, p1)
        torch.testing.assert_close(lg[0, -1], want, atol=2e-4, rtol=2e-4)


# ------------------------------------------------------------------------------------ CLI
def test_cli_switch_parses_and_defaults_to_cap():
    from src.main import _executor_kwargs, build_parser

    base = ["--model", "mistral-7b", "--splits", "16", "--stage", "1"]
    a = build_parser().parse_args(base)
    assert a.sliding_window == "cap" and "sliding_window" not in _executor_kwargs(a)
    a = build_parser().parse_args(base + ["--sliding_window", "attend"])
    assert a.sliding_window == "attend" and _executor_kwargs(a)["sliding_window"] == "attend"
    with pytest.raises(SystemExit):
        build_parser().parse_args(base + ["--sliding_window", "full"])


@pytest.mark.timeout(120)
def test_stage_server_with_attend_reports_the_window_and_generates():
    """``--sliding_window attend`` on a stage server (CPU): ``rpc_info`` and the announcement carry the
    mode and W, and the client's greedy tokens come out of the served span."""
    from src import main as M
    from src.comm.wire import Message
    from src.dht_utils import get_stage_key

    from .swarm_utils import ServerThread, client_args, server_argv

    model, cut = "tiny-mistral", 2
    s1 = ServerThread(server_argv(model, str(cut), 1, extra="--sliding_window attend")).wait()
    try:
        ex = s1.srv.ex
        assert ex.window == 96 and ex.sliding_window == "attend" and ex.max_seq_len == 1024
        info = s1.srv.loop.run(s1.srv.handler.rpc_info(Message({}, [])), timeout=10)
        assert info.metadata["sliding_window"] == "attend" and info.metadata["window"] == 96
        rec = s1.dht.get(get_stage_key(1), latest=True)
        assert "sliding_window" in repr(rec.value) and "attend" in repr(rec.value)
        args = client_args(model, str(cut), s1.addr, "--max_new_tokens 6 --temperature 0 --sliding_window attend")
        gen = M.run_rank0(args, torch.device("cpu"), [cut])
    finally:
        s1.close()
    assert len(gen) == 6
