"""ops.sample_verify on the GPU against an oracle composed from ops.sample, bit for bit.

The oracle draws block column j of every session with ONE ops.sample call over S rows: row s holds
session s's logits row j, the history (h_s + draft_s[:j])[-RECENT:] expanded on the host and that
row's seed - what a one-token step of the same sessions in the same order would sample.  The
accept scan (leading draws equal to their draft, plus one) runs in numpy."""
import numpy as np
import pytest
import torch

from src import ops
from src.runtime.sampler import RECENT

pytestmark = pytest.mark.gpu

DEV = "cuda"
# rows per session (K_s + 1), R <= 64: one session at every block width, equal and ragged blocks
# over 3 sessions, 16 sessions without drafts, with one draft each, and ragged
SHAPES = {
    "s1_k0": [1], "s1_k1": [2], "s1_k4": [5], "s1_k15": [16],
    "s3_ragged": [5, 1, 16], "s3_k1": [2, 2, 2], "s3_k15": [16, 16, 16],
    "s16_k0": [1] * 16, "s16_k1": [2] * 16, "s16_ragged": [5, 1, 2, 5, 1, 2, 5, 16, 1, 2, 5, 1, 2, 5, 1, 2],
}
VOCABS = [512, 32000, 128256]  # tiny models; Llama-2 (one workgroup per row); Llama-3 (the split path)


def _params(S, g, greedy):
    """Per-session parameters that reach every sampler path: top-k 50 / 5 (fast path, and the split
    path at the wide vocabulary), 100 (> the split path's 64: its rows fall back to the one-workgroup
    kernel), 0 (the general path), with and without top-p and repetition penalty; greedy sessions mixed in."""
    ks = [50, 0, 5, 100]
    temps = np.array([0.0 if greedy == "all" or (greedy == "mixed" and s % 5 == 4) else (0.7 + 0.1 * (s % 4))
                      for s in range(S)], dtype=np.float32)
    top_ps = np.array([(0.92, 1.0, 0.5, 0.9)[s % 4] for s in range(S)], dtype=np.float32)
    top_ks = np.array([ks[(s + s // 4) % 4] for s in range(S)], dtype=np.int32)
    reps = np.array([(1.5, 1.0, 1.2, 1.5)[(s + 1) % 4] for s in range(S)], dtype=np.float32)
    return temps, top_ps, top_ks, reps


def _hist(s, V, g):
    """Histories: empty, short, 48 ids (the window slides inside a block of 4 drafts), full."""
    n = (0, 3, 48, RECENT)[s % 4]
    return torch.randint(0, V, (n,), generator=g).tolist()


def _pack_hist(hs):
    rec = np.zeros((len(hs), RECENT), dtype=np.int32)
    ln = np.zeros(len(hs), dtype=np.int32)
    for s, h in enumerate(hs):
        h = list(h)[-RECENT:]
        ln[s] = len(h)
        rec[s, :len(h)] = h
    return rec, ln


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _case(V, rows, greedy="mixed", seed=0):
    """Build a case and its oracle.  Session s's drafts follow its mode (s % 4): every draft right;
    wrong at row 0; wrong in the middle; one random id drafted again and again (as good as always
    rejected at row 0: the accepted repeated drafts are ``test_sample_verify_last_three_rule``)."""
    g = torch.Generator().manual_seed(1000 * seed + V % 977 + len(rows))
    S, R = len(rows), sum(rows)
    row_start = np.zeros(S + 1, dtype=np.int32)
    row_start[1:] = np.cumsum(rows)
    logits = (3.0 * torch.randn(R, V, generator=g)).to(torch.bfloat16).to(DEV)
    seeds = torch.randint(0, 2 ** 62, (R,), generator=g).numpy().astype(np.int64)
    hists = [_hist(s, V, g) for s in range(S)]
    temps, top_ps, top_ks, reps = _params(S, g, greedy)
    dp = [_dev(a) for a in (temps, top_ps, top_ks, reps)]
    drafts = [[] for _ in range(S)]
    draws = [[] for _ in range(S)]
    rep_id = int(torch.randint(0, V, (1,), generator=g))
    for j in range(max(rows)):
        live = [s for s in range(S) if j < rows[s]]
        lg = torch.zeros(S, V, dtype=torch.bfloat16, device=DEV)
        sd = np.zeros(S, dtype=np.int64)
        hs = [[] for _ in range(S)]
        for s in live:
            lg[s] = logits[row_start[s] + j]
            sd[s] = seeds[row_start[s] + j]
            hs[s] = (hists[s] + drafts[s][:j])[-RECENT:]
        rec, ln = _pack_hist(hs)
        out = ops.sample(lg, dp[0], dp[1], dp[2], dp[3], _dev(rec), _dev(ln), _dev(sd)).tolist()
        for s in live:
            t = int(out[s])
            draws[s].append(t)
            if j < rows[s] - 1:
                mode, K = s % 4, rows[s] - 1
                wrong = (mode == 1 and j == 0) or (mode == 2 and j == K // 2)
                drafts[s].append(rep_id if mode == 3 else ((t + 1) % V if wrong else t))
    # the accept scan
    tokens = np.full(R, -1, dtype=np.int64)
    count = np.zeros(S, dtype=np.int32)
    for s in range(S):
        n = 0
        while n < rows[s] - 1 and draws[s][n] == drafts[s][n]:
            n += 1
        count[s] = n + 1
        tokens[row_start[s]:row_start[s] + n + 1] = draws[s][:n + 1]
    draft = np.full(R, -1, dtype=np.int32)
    for s in range(S):
        draft[row_start[s]:row_start[s] + rows[s] - 1] = drafts[s]
    return dict(logits=logits, row_start=row_start, draft=draft, seeds=seeds, hists=hists, dp=dp, tokens=tokens,
                count=count, S=S, R=R, V=V)


def _verify(c, update, all_greedy=False):
    rec, ln = _pack_hist(c["hists"])
    recent, rlen = _dev(rec), _dev(ln)
    tokens = torch.full((c["R"] + 8,), -7, dtype=torch.long, device=DEV)  # sentinels behind R / S
    count = torch.full((c["S"] + 4,), -7, dtype=torch.int32, device=DEV)
    ops.sample_verify(c["logits"], _dev(c["row_start"]), _dev(c["draft"]), *c["dp"], recent, rlen, _dev(c["seeds"]),
                      tokens=tokens, count=count, update_history=update, all_greedy=all_greedy)
    return tokens.cpu().numpy(), count.cpu().numpy(), recent.cpu().numpy(), rlen.cpu().numpy()


def _check(c, all_greedy=False):
    for update in (False, True):
        tokens, count, recent, rlen = _verify(c, update, all_greedy)
        R, S = c["R"], c["S"]
        assert np.array_equal(tokens[:R], c["tokens"]), (update, tokens[:R].tolist(), c["tokens"].tolist())
        assert np.array_equal(count[:S], c["count"])
        assert (tokens[R:] == -7).all() and (count[S:] == -7).all()
        for s in range(S):
            lo = c["row_start"][s]
            kept = c["tokens"][lo:lo + c["count"][s]].tolist()
            want = (c["hists"][s] + kept)[-RECENT:] if update else c["hists"][s][-RECENT:]
            assert rlen[s] == len(want) and recent[s, :len(want)].tolist() == want, (s, update)


@pytest.mark.parametrize("V", VOCABS)
@pytest.mark.parametrize("shape", sorted(SHAPES))
def test_sample_verify_matches_composed_oracle(V, shape):
    c = _case(V, SHAPES[shape])
    _check(c)
    if shape == "s3_ragged":  # the acceptance cases are what they are meant to be
        assert c["count"][0] == 5 and c["count"][1] == 1 and 1 < c["count"][2] < 16
    if shape == "s3_k1":
        assert c["count"][0] == 2 and c["count"][1] == 1


@pytest.mark.parametrize("V", VOCABS)
def test_sample_verify_without_drafts_is_sample(V):
    c = _case(V, [1] * 16, seed=1)
    rec, ln = _pack_hist(c["hists"])
    for update in (False, True):
        recent, rlen = _dev(rec), _dev(ln)
        want = ops.sample(c["logits"], *c["dp"], recent, rlen, _dev(c["seeds"]), update_history=update)
        tokens, count, recent2, rlen2 = _verify(c, update)
        assert np.array_equal(tokens[:16], want.cpu().numpy()) and (count[:16] == 1).all()
        assert np.array_equal(recent2, recent.cpu().numpy()) and np.array_equal(rlen2, rlen.cpu().numpy())


@pytest.mark.parametrize("V", VOCABS)
def test_sample_verify_all_greedy(V):
    """Every temperature <= 0: the same answer through the sampler's argmax rows and with ``all_greedy``."""
    c = _case(V, [5, 1, 16, 2], greedy="all", seed=2)
    want = c["logits"].float().cpu().numpy().argmax(-1)  # (numpy: the first maximum, as the kernels take)
    for s in range(c["S"]):
        lo = c["row_start"][s]
        assert np.array_equal(c["tokens"][lo:lo + c["count"][s]], want[lo:lo + c["count"][s]])
    _check(c)
    _check(c, all_greedy=True)


@pytest.mark.parametrize("top_k", [0, 50])
@pytest.mark.parametrize("V", [512, 128256])
def test_sample_verify_last_three_rule(V, top_k):
    """Drafts that repeat one id three times and are accepted: row 3 is drawn against a window ending
    in three equal drafted ids, and draws the rival id only if the expand kernel's window carries the
    last-three rule (``last_three_case`` in test_speculative.py has the arithmetic).  top_k 0: the
    general path; 50: the fast path, and the split path at the wide vocabulary."""
    from .test_speculative import last_three_case

    logits, blocks, hists, want = last_three_case(V)
    S, R = 2, 5
    f = lambda v, dt=np.float32: _dev(np.full(S, v, dtype=dt))  # noqa: E731
    dp = [f(1e-3), f(1.0), f(top_k, np.int32), f(1.5)]
    draft = np.array([9, 9, 9, -1, -1], dtype=np.int32)
    for update in (False, True):
        rec, ln = _pack_hist(hists)
        recent, rlen = _dev(rec), _dev(ln)
        tokens, count = ops.sample_verify(logits.to(torch.bfloat16).to(DEV), _dev(np.array([0, 4, 5], dtype=np.int32)),
                                          _dev(draft), *dp, recent, rlen, _dev(np.arange(R, dtype=np.int64)),
                                          update_history=update)
        assert tokens.tolist() == want[0] + want[1] and count.tolist() == [4, 1]
        if update:
            assert recent[0, :4].tolist() == [9, 9, 9, 10] and rlen.tolist() == [4, 5]
            assert recent[1, :5].tolist() == [9, 9, 9, 4, 9]
