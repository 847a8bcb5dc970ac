"""Speculative decoding on the CPU data path: the verify sampler's reference semantics, all-row
logits of the executor, verify requests on the handler, and the client's accept loop over a
localhost swarm (same output as the plain loop, with drafters that are right, wrong and half right)."""
import logging
import math

import pytest
import torch

from src import main as M
from src.comm.wire import Message
from src.dht_utils import get_stage_key
from src.models.config import resolve_model
from src.models.weights import random_stage_weights
from src.ops import reference as ref
from src.rpc_handler import StageConnectionHandler
from src.runtime.executor import StageExecutor
from src.runtime.sampler import RECENT
from src.runtime.speculative import NgramDrafter, speculative_generate

from .swarm_utils import ServerThread, client_args, server_argv, wait_for

V = 64
PARAMS = dict(temp=0.9, top_p=0.95, top_k=8, rp=1.3)


# ------------------------------------------------------------------ reference.sample_verify
def _hand_loop(logits, rows, drafts, hist, seeds, p=PARAMS):
    """Row j by ``sample_row`` on (hist + drafts[:j])[-RECENT:]; keep the leading matches and one more."""
    kept = []
    for j, row in enumerate(rows):
        g = torch.Generator().manual_seed(int(seeds[row]))
        t = ref.sample_row(logits[row], p["temp"], p["top_p"], p["top_k"], p["rp"],
                           (list(hist) + list(drafts[:j]))[-RECENT:], generator=g)
        kept.append(t)
        if j == len(drafts) or t != drafts[j]:
            break
    return kept


def _draws(logits, rows, hist, seeds, k, p=PARAMS):
    """The k tokens a plain loop would draw from these rows: the drafts that are all accepted."""
    out = []
    for j in range(k):
        g = torch.Generator().manual_seed(int(seeds[rows[j]]))
        out.append(ref.sample_row(logits[rows[j]], p["temp"], p["top_p"], p["top_k"], p["rp"],
                                  (list(hist) + out)[-RECENT:], generator=g))
    return out


def _call(logits, blocks, hists, seeds, update=False, p=PARAMS):
    S = len(blocks)
    row_start = torch.zeros(S + 1, dtype=torch.int32)
    row_start[1:] = torch.cumsum(torch.tensor([len(d) + 1 for d in blocks]), 0)
    draft = torch.full((int(row_start[-1]),), -1, dtype=torch.int32)
    for s, d in enumerate(blocks):
        draft[int(row_start[s]):int(row_start[s]) + len(d)] = torch.tensor(d, dtype=torch.int32)
    recent = torch.zeros(S, RECENT, dtype=torch.int32)
    rlen = torch.zeros(S, dtype=torch.int32)
    for s, h in enumerate(hists):
        h = list(h)[-RECENT:]
        rlen[s] = len(h)
        recent[s, :len(h)] = torch.tensor(h, dtype=torch.int32)
    f = lambda v: torch.full((S,), v, dtype=torch.float32)  # noqa: E731
    toks, cnt = ref.sample_verify(logits, row_start, draft, f(p["temp"]), f(p["top_p"]),
                                  torch.full((S,), p["top_k"], dtype=torch.int32), f(p["rp"]), recent, rlen, seeds,
                                  update_history=update)
    return toks, cnt, row_start.tolist(), recent, rlen


def _wrong(t):
    return (t + 1) % V


def test_reference_sample_verify_matches_hand_loop():
    g = torch.Generator().manual_seed(11)
    # sessions: accept all (K=4), reject at row 0 (K=3), reject in the middle (K=4), K=0,
    # a 48-token history + 4 accepted drafts (the window slides), one id drafted three times over random
    # logits (rejected at row 0; the block whose repeated drafts ARE accepted is the next test)
    K = [4, 3, 4, 0, 4, 3]
    R = sum(k + 1 for k in K)
    logits = 3.0 * torch.randn(R, V, generator=g)
    seeds = torch.randint(0, 2 ** 40, (R,), generator=g)
    hists = [[1, 2, 3], [4, 5], [7, 7, 9], [3], torch.randint(0, V, (48,), generator=g).tolist(), [5, 6]]
    starts = [0]
    for k in K:
        starts.append(starts[-1] + k + 1)
    rows = [list(range(starts[s], starts[s + 1])) for s in range(len(K))]
    blocks = []
    for s, k in enumerate(K):
        d = _draws(logits, rows[s], hists[s], seeds, k)
        if s == 1:
            d[0] = _wrong(d[0])
        elif s == 2:
            d[2] = _wrong(d[2])
        elif s == 5:
            d = [9, 9, 9]
        blocks.append(d)
    toks, cnt, rs, _, _ = _call(logits, blocks, hists, seeds)
    want_counts = []
    for s in range(len(K)):
        kept = _hand_loop(logits, rows[s], blocks[s], hists[s], seeds)
        want_counts.append(len(kept))
        got = toks[rs[s]:rs[s + 1]].tolist()
        assert got == kept + [-1] * (K[s] + 1 - len(kept)), f"session {s}"
    assert cnt.tolist() == want_counts
    assert want_counts == [5, 1, 3, 1, 5, 1]


NEAR_GREEDY = dict(temp=1e-3, top_p=1.0, top_k=0, rp=1.5)  # the larger penalised logit is drawn


def last_three_case(vocab):
    """A block whose drafts repeat id 9 three times and are all accepted, so that row 3 is drawn
    against a window that ends in three equal DRAFTED ids.  Logit 8 for id 9 on every row, a rival
    id 10 that no history holds.  Row j sees j nines: 8 / 1.5**j = 8, 5.33, 3.56 beats the rival's 1.0
    on rows 0..2.  Row 3 sees three nines: the count penalty alone leaves 8 / 1.5**3 = 2.37, the
    last-three rule's further rp**3 leaves 0.70; the rival's 1.5 lies between, so row 3 draws 10 iff
    the rule is applied over the drafted window.  A control session without drafts, history
    [9, 9, 9, 4] (three nines, not the last three), draws 9 from the same row.
    Returns (logits [5, vocab], drafts per session, histories, expected tokens per session)."""
    logits = torch.zeros(5, vocab)
    logits[:, 9] = 8.0
    logits[:3, 10] = 1.0
    logits[3:, 10] = 1.5
    return logits, [[9, 9, 9], []], [[], [9, 9, 9, 4]], [[9, 9, 9, 10], [9]]


def test_reference_sample_verify_last_three_rule_over_accepted_drafts():
    logits, blocks, hists, want = last_three_case(V)
    for update in (False, True):
        toks, cnt, rs, recent, rlen = _call(logits, blocks, hists, torch.arange(5), update=update, p=NEAR_GREEDY)
        assert cnt.tolist() == [4, 1]
        assert toks.tolist() == want[0] + want[1]
        if update:
            assert recent[0, :4].tolist() == [9, 9, 9, 10] and rlen.tolist() == [4, 5]
    # without the rule's term row 3 would keep drawing 9: the case tells the two apart
    g = torch.Generator().manual_seed(0)
    assert ref.sample_row(logits[3], 1e-3, 1.0, 0, 1.5, [9, 9, 9, 4], generator=g) == 9


def test_reference_sample_verify_window_slides_over_accepted_drafts():
    """A full window whose oldest id is 9: row 0 still sees it (9 is penalised, the rival 10 is drawn
    and accepted), row 1's window has lost it (9 is unpenalised again and drawn)."""
    logits = torch.zeros(2, V)
    logits[:, 9] = 2.0
    logits[:, 10] = 1.9
    toks, cnt, _, _, _ = _call(logits, [[10]], [[9] + [20] * 49], torch.tensor([1, 2]), p=NEAR_GREEDY)
    assert toks.tolist() == [10, 9] and cnt.tolist() == [2]


@pytest.mark.parametrize("update", [False, True])
def test_reference_sample_verify_pushes_exactly_count(update):
    g = torch.Generator().manual_seed(5)
    logits = 3.0 * torch.randn(5, V, generator=g)
    seeds = torch.randint(0, 2 ** 40, (5,), generator=g)
    hist = torch.randint(0, V, (49,), generator=g).tolist()
    d = _draws(logits, list(range(5)), hist, seeds, 4)
    d[2] = _wrong(d[2])
    toks, cnt, _, recent, rlen = _call(logits, [d], [hist], seeds, update=update)
    assert cnt.tolist() == [3]
    kept = toks[:3].tolist()
    want = (hist + kept)[-RECENT:] if update else hist
    assert rlen.tolist() == [len(want)] and recent[0, :len(want)].tolist() == want


# ------------------------------------------------------------------ executor: logit_rows
def _ex(model, **kw):
    cfg = resolve_model(model)
    w = random_stage_weights(cfg, 0, cfg.num_hidden_layers, has_embed=True, has_head=True, device="cpu",
                             dtype=torch.float32, seed=7)
    kw.setdefault("max_seq_len", 256)
    return cfg, StageExecutor(cfg, w, "cpu", dtype=torch.float32, kv_cache_bytes=32 << 20, max_sessions=8, **kw)


@pytest.mark.parametrize("model", ["tiny-llama", "tiny-gpt2"])
def test_logit_rows_equal_one_token_steps(model):
    cfg, ex = _ex(model)
    g = torch.Generator().manual_seed(2)
    ids = torch.randint(0, cfg.vocab_size, (70,), generator=g)  # the block 62..66 crosses the 64-token page
    ex.forward([("a", 62)], ids[:62])
    ex.forward([("b", 62)], ids[:62])
    got = ex.forward([("a", 5)], ids[62:67], logit_rows=[5])
    assert got.shape == (5, cfg.vocab_size)
    for j in range(5):
        one = ex.forward([("b", 1)], ids[62 + j:63 + j])
        torch.testing.assert_close(got[j:j + 1], one, atol=1e-5, rtol=1e-5)
    # a ragged step: 3 trailing rows of one sequence, the last row of another
    ex.forward([("c", 67)], ids[:67])
    rag = ex.forward([("a", 3), ("c", 2)], torch.cat([ids[67:70], ids[67:69]]), logit_rows=[3, 1])
    assert rag.shape == (4, cfg.vocab_size)
    for j in range(3):
        one = ex.forward([("b", 1)], ids[67 + j:68 + j])
        torch.testing.assert_close(rag[j:j + 1], one, atol=1e-5, rtol=1e-5)
        if j == 1:
            torch.testing.assert_close(rag[3:4], one, atol=1e-5, rtol=1e-5)  # c's last row: position 68


@pytest.mark.parametrize("model", ["tiny-llama", "tiny-gpt2"])
def test_logit_rows_default_unchanged(model):
    cfg, ex = _ex(model)
    ids = torch.arange(20) % cfg.vocab_size
    a = ex.forward([("a", 12), ("b", 8)], ids)
    b = ex.forward([("c", 12), ("d", 8)], ids, logit_rows=None)
    c = ex.forward([("e", 12), ("f", 8)], ids, logit_rows=[1, 1])
    assert a.shape == (2, cfg.vocab_size) and torch.equal(a, b) and torch.equal(a, c)
    with pytest.raises(ValueError):
        ex.forward([("g", 4)], ids[:4], logit_rows=[5])
    with pytest.raises(ValueError):
        ex.forward([("g", 4)], ids[:4], logit_rows=[1, 1])


def test_logit_rows_chunked_step():
    cfg, big = _ex("tiny-llama")
    _, small = _ex("tiny-llama", max_tokens_per_step=7)
    ids = torch.arange(20) * 3 % cfg.vocab_size
    want = big.forward([("a", 20)], ids, logit_rows=[4])
    got = small.forward([("a", 20)], ids, logit_rows=[4])  # chunks of 7, 7, 6: the 4 rows are in the last
    torch.testing.assert_close(got, want, atol=1e-4, rtol=1e-4)
    with pytest.raises(ValueError, match="last chunk"):
        small.forward([("b", 20)], ids, logit_rows=[7])


# ------------------------------------------------------------------ handler
def _msg(sid, ids, cur_len, prefill=False, drafts=None, gen=()):
    md = {"session_id": sid, "cur_len": cur_len, "is_prefill": prefill, "temperature": 0.0,
          "generated_tokens": list(gen)}
    if drafts is not None:
        md["draft_tokens"] = list(drafts)
    return Message(md, [torch.tensor([ids], dtype=torch.long)])


def test_handler_mixed_batch_with_verify_requests(caplog):
    cfg, ex = _ex("tiny-llama")
    _, solo = _ex("tiny-llama")
    h = StageConnectionHandler(None, ex, final_stage=True)
    g = torch.Generator().manual_seed(3)
    prompt = {s: torch.randint(0, cfg.vocab_size, (n,), generator=g).tolist()
              for s, n in (("p", 9), ("d", 6), ("v1", 7), ("v2", 5))}
    # the greedy continuation of every session, one token at a time on a second executor
    plain = {}
    for s, p in prompt.items():
        t = int(torch.argmax(solo.forward([(s, len(p))], torch.tensor(p))[-1]))
        plain[s] = [t]
        for _ in range(5):
            t = int(torch.argmax(solo.forward([(s, 1)], torch.tensor([t]))[-1]))
            plain[s].append(t)
    try:
        for s in ("d", "v1", "v2"):
            r = h._run_batch([h._parse(_msg(s, prompt[s], len(prompt[s]), prefill=True))])[0]
            assert r.metadata["token_id"] == plain[s][0] and "token_ids" not in r.metadata
        d1 = plain["v1"][1:4]                      # K = 3, every draft right
        d2 = [(plain["v2"][1] + 1) % cfg.vocab_size, 0]  # K = 2, wrong at once
        L = {s: len(p) for s, p in prompt.items()}
        batch = [h._parse(_msg("p", prompt["p"], L["p"], prefill=True)),
                 h._parse(_msg("d", [plain["d"][0]], L["d"] + 1, gen=plain["d"][:1])),
                 h._parse(_msg("v1", [plain["v1"][0]] + d1, L["v1"] + 4, drafts=d1, gen=plain["v1"][:1])),
                 h._parse(_msg("v2", [plain["v2"][0]] + d2, L["v2"] + 3, drafts=d2, gen=plain["v2"][:1]))]
        rp, rd, r1, r2 = h._run_batch(batch)
        assert rp.metadata["token_id"] == plain["p"][0] and tuple(rp.tensors[0].shape) == (1, 1)
        assert rd.metadata["token_id"] == plain["d"][1] and "token_ids" not in rd.metadata
        assert r1.metadata["token_ids"] == plain["v1"][1:5] and tuple(r1.tensors[0].shape) == (1, 4)
        assert r2.metadata["token_ids"] == plain["v2"][1:2] and tuple(r2.tensors[0].shape) == (1, 1)
        for r in (r1, r2):
            assert r.metadata["token_id"] == r.metadata["token_ids"][0]
            assert r.tensors[0].reshape(-1).tolist() == r.metadata["token_ids"]
        # sessions are left at start + K + 1; the next request's cur_len rewinds without a warning
        assert ex.sessions.get("v1").length == L["v1"] + 4 and ex.sessions.get("v2").length == L["v2"] + 3
        with caplog.at_level(logging.WARNING):
            nxt = h._parse(_msg("v2", [plain["v2"][1]], L["v2"] + 2, gen=plain["v2"][:2]))
            assert nxt.start == L["v2"] + 1
            r = h._run_batch([nxt])[0]
        assert r.metadata["token_id"] == plain["v2"][2]
        assert ex.sessions.get("v2").length == L["v2"] + 2
        assert not [rec for rec in caplog.records if "mismatch" in rec.getMessage()]
        with pytest.raises(ValueError, match="draft_tokens"):
            h._parse(_msg("v1", [1, 2, 3], L["v1"] + 7, drafts=[2]))
        for bad in (cfg.vocab_size, -1, 2 ** 31):  # refused per request, before it joins a batch
            with pytest.raises(ValueError, match="vocabulary"):
                h._parse(_msg("v1", [1, 2], L["v1"] + 6, drafts=[bad]))
    finally:
        h.shutdown()


def test_handler_refuses_drafts_on_a_rolling_window_stage():
    cfg = resolve_model("tiny-mistral")
    w = random_stage_weights(cfg, 0, cfg.num_hidden_layers, has_embed=True, has_head=True, device="cpu",
                             dtype=torch.float32, seed=7)
    ex = StageExecutor(cfg, w, "cpu", dtype=torch.float32, kv_cache_bytes=32 << 20, max_sessions=4, max_seq_len=256,
                       sliding_window="attend")
    h = StageConnectionHandler(None, ex, final_stage=True)
    try:
        h._run_batch([h._parse(_msg("s", [1, 2, 3], 3, prefill=True))])
        with pytest.raises(ValueError, match="draft_tokens with --sliding_window attend"):
            h._parse(_msg("s", [4, 5], 5, drafts=[5]))
    finally:
        h.shutdown()


# ------------------------------------------------------------------ client
def test_ngram_drafter_prompt_lookup():
    d = NgramDrafter()
    assert d.propose([1, 2, 3, 4, 5, 1, 2], [3], 3) == [4, 5, 1]       # suffix (1, 2, 3) seen before
    assert d.propose([1, 2, 3, 9, 2, 3, 7], [8, 2, 3], 2) == [7, 8]     # the most recent earlier occurrence
    assert d.propose([1, 2, 3], [4], 4) == []                           # no match: a plain step
    assert d.propose([5, 6, 5], [], 4) == [6, 5]                        # fewer than k tokens follow
    assert d.propose([5, 6, 5], [], 0) == []


def test_accept_loop_follows_the_plain_stop_rules():
    """A scripted model: token i of the stream is fixed; the loop must emit the plain loop's prefix."""
    for stream, eos in (([3, 4, 5, 9, 6, 7], 9), ([3, 4, 4, 4, 4, 4, 4, 4, 8], None), (list(range(10, 30)), None)):
        def plain(n):
            out, rep, last = [stream[0]], 0, None
            for t in stream[1:n]:
                if out[-1] == eos or t == eos:
                    break
                if t == last:
                    rep += 1
                    if rep >= 5:
                        break
                else:
                    rep, last = 0, t
                out.append(t)
            return out

        class Oracle:
            def propose(self, prompt, generated, k):
                return stream[len(generated):len(generated) + k]

        def verify(tokens, cur_len, generated):
            pos = len(generated)
            assert cur_len == 2 + pos + len(tokens) - 1 and tokens[0] == generated[-1]
            kept = []
            for j, d in enumerate(tokens[1:] + [None]):
                kept.append(stream[pos + j])
                if kept[-1] != d:
                    break
            return kept

        for n in (1, 2, 6, 9):
            gen, stats = speculative_generate(stream[0], [0, 0], n, 3, Oracle(), lambda t, c, g_: stream[len(g_)],
                                              verify, eos=eos, max_length=2 + n)
            assert gen == plain(n), (stream, n)
            assert stats.accepted == stats.drafted


def test_verify_reply_without_token_ids_is_an_error():
    """A final stage that ignores draft_tokens samples the block's last row only: its token_id is not t_0."""
    import time
    import types

    from src.rpc_transport import RpcTransport

    tx = types.SimpleNamespace(last_decode_stage_times=None, last_decode_total=None, decode_stage_history=[],
                               decode_total_times=[], _token_of=RpcTransport._token_of)
    ok = Message({"token_id": 3, "token_ids": [3, 4]}, [torch.tensor([[3, 4]])])
    assert RpcTransport._finish(tx, "verify", [("hop", 0.1)], time.perf_counter(), ok) == [3, 4]
    assert len(tx.decode_stage_history) == 1  # verify steps count among the per-hop decode timings
    with pytest.raises(RuntimeError, match="token_ids"):
        RpcTransport._finish(tx, "verify", [], time.perf_counter(), Message({"token_id": 3}, [torch.tensor([[3]])]))


MODEL = "tiny-llama"
SAMPLING = {"greedy": "--temperature 0", "cli": ""}  # "": the CLI's temperature 1.0 / top_p 0.92 / top_k 50


PLAIN_KEYS = {"session_id", "seq_len", "cur_len", "is_prefill", "max_length", "temperature", "top_p", "top_k",
              "generated_tokens"}


class _Oracle:
    def __init__(self, plain):
        self.plain = plain

    def propose(self, prompt_ids, generated, k):
        return self.plain[len(generated):len(generated) + k]


class _Wrong(_Oracle):
    def propose(self, prompt_ids, generated, k):
        return [(t + 1) % 512 for t in super().propose(prompt_ids, generated, k)]


class _TwoRight(_Oracle):
    def propose(self, prompt_ids, generated, k):
        d = super().propose(prompt_ids, generated, k)
        return d[:2] + [(t + 1) % 512 for t in d[2:]]


def _run(peers, extra, **kw):
    args = client_args(MODEL, "1,3", peers, "--max_new_tokens 16 --device_channel off " + extra)
    return M.run_rank0(args, torch.device("cpu"), [1, 3], session_id="spec-test-session", **kw)


@pytest.mark.timeout(180)
@pytest.mark.parametrize("sampling", sorted(SAMPLING))
def test_swarm_speculative_output_equals_plain(sampling):
    s1 = ServerThread(server_argv(MODEL, "1,3", 1)).wait()
    s2 = ServerThread(server_argv(MODEL, "1,3", 2, peers=s1.addr)).wait()
    try:
        assert wait_for(lambda: s1.dht.get(get_stage_key(2)) is not None)
        seen = []  # metadata keys of the requests that reach the final stage
        parse = s2.srv.handler._parse
        s2.srv.handler._parse = lambda msg: (seen.append(set(msg.metadata)), parse(msg))[1]
        plain = _run(s1.addr, SAMPLING[sampling])
        assert len(plain) > 6, "the plain run stopped too early to say anything"
        # --speculative_tokens 0 sends the requests it always sent: no new metadata key
        assert seen and set().union(*seen) == PLAIN_KEYS
        del seen[:]
        for drafter, accept_all in ((_Oracle(plain), True), (_Wrong(plain), False), (_TwoRight(plain), False)):
            res = []
            gen = _run(s1.addr, SAMPLING[sampling] + " --speculative_tokens 4", drafter=drafter, results=res)
            assert gen == plain, type(drafter).__name__
            stats = res[-1]
            assert any("draft_tokens" in k for k in seen) and set().union(*seen) == PLAIN_KEYS | {"draft_tokens"}
            if accept_all:  # every draft accepted: 5 tokens per step
                assert stats.accepted == stats.drafted > 0
                assert stats.steps == math.ceil((len(plain) - 1) / 5)
            elif isinstance(drafter, _Wrong):
                assert stats.accepted == 0 and stats.drafted > 0
                assert stats.tokens == stats.steps
            else:
                assert 0 < stats.accepted < stats.drafted
                assert stats.steps < len(plain) - 1
    finally:
        s1.close()
        s2.close()


@pytest.mark.timeout(180)
def test_swarm_speculative_failover_replays_accepted_rows():
    s1 = ServerThread(server_argv(MODEL, "1,3", 1)).wait()
    s2 = ServerThread(server_argv(MODEL, "1,3", 2, peers=s1.addr)).wait()
    s2b = ServerThread(server_argv(MODEL, "1,3", 2, peers=s1.addr)).wait()
    try:
        assert wait_for(lambda: len(s1.dht.get(get_stage_key(2)).value) == 2)
        plain = _run(s1.addr, "--temperature 0")
        killed = []
        before = {s: s.srv.handler.stats["requests"] for s in (s2, s2b)}

        def kill_final(i):
            if i == 2 and not killed:  # after two blocks of two accepted and two rejected drafts
                # the final stage that holds the session is the one that has served this run's requests
                victim = s2 if s2.srv.handler.stats["requests"] > before[s2] else s2b
                victim.kill()
                killed.append(victim)

        gen = _run(s1.addr, "--temperature 0 --speculative_tokens 4", drafter=_TwoRight(plain), on_step=kill_final)
        assert killed, "no server was killed"
        assert gen == plain
    finally:
        for s in (s1, s2, s2b):
            s.close()


@pytest.mark.parametrize("extra, what", [("--push", "--push"), ("--num_sessions 2", "--num_sessions"),
                                         ("--device_channel on", "device channel"),
                                         ("--model tiny-mistral --sliding_window attend", "sliding-window")])
def test_unbuilt_combinations_raise_at_start_up(extra, what):
    args = client_args(MODEL, "1,3", "/ip4/127.0.0.1/tcp/1", "--speculative_tokens 4 " + extra)
    with pytest.raises(ValueError, match=what):
        M.run_rank0(args, torch.device("cpu"), [1, 3])


def test_cli_default_is_the_plain_loop():
    args = client_args(MODEL, "1,3", "/ip4/127.0.0.1/tcp/1")
    assert args.speculative_tokens == 0 and args.draft == "ngram"
