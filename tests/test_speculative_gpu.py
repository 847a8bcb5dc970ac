"""Speculative verify steps on the GPU executor: all-row logits, the rewind after a rejected block,
and greedy blocks end to end (executor + BatchSampler.verify) on a last-stage executor."""
import pytest
import torch

from src.models.config import resolve_model
from src.models.reference_model import reference_forward
from src.models.weights import random_stage_weights
from src.runtime.executor import StageExecutor
from src.runtime.sampler import BatchSampler, SamplingParams

pytestmark = pytest.mark.gpu

MODELS = ["small-llama", "tiny-llama"]
KV = ["bf16", "fp8"]
_W = {}


def _weights(model):
    if model not in _W:
        cfg = resolve_model(model)
        _W[model] = (cfg, random_stage_weights(cfg, 0, cfg.num_hidden_layers, has_embed=True, has_head=True,
                                               device="cuda", dtype=torch.bfloat16, seed=3))
    return _W[model]


def _ex(model, kv, **kw):
    cfg, w = _weights(model)
    if kv != "bf16":
        kw["kv_cache_dtype"] = kv
    return cfg, w, StageExecutor(cfg, w, "cuda", kv_cache_bytes=64 << 20, max_sessions=8, max_seq_len=256, **kw)


def _ids(cfg, n, seed=0):
    return torch.randint(0, cfg.vocab_size, (n,), generator=torch.Generator().manual_seed(seed)).cuda()


@pytest.mark.parametrize("kv", KV)
@pytest.mark.parametrize("model", MODELS)
def test_all_row_logits_of_a_verify_step(model, kv):
    """A 5-token verify step at positions 62..66 of a 70-token context (the 64-token page boundary is
    inside the block) against the fp32 oracle, with the bound of test_executor_gpu's prefill logits."""
    cfg, w, ex = _ex(model, kv)
    ids = _ids(cfg, 70)
    ex.forward([("a", 62), ("b", 62)], torch.cat([ids[:62], ids[:62]]))
    got = ex.forward([("a", 5)], ids[62:67], logit_rows=[5])
    assert got.shape == (5, cfg.vocab_size)
    last = ex.forward([("b", 5)], ids[62:67])
    assert torch.equal(got[4:5], last)  # the last row is the plain step's logits, bit for bit
    want = reference_forward([w], ids[:67])[62:67]
    print(f"{model} kv={kv}: max |logit error| {float((got.float() - want).abs().max()):.4f}")
    torch.testing.assert_close(got.float(), want, atol=0.06, rtol=0.05)
    # the three remaining tokens as a ragged step next to a sequence that wants one row
    rag = ex.forward([("a", 3), ("b", 3)], torch.cat([ids[67:70], ids[67:70]]), logit_rows=[3, 1])
    assert rag.shape == (4, cfg.vocab_size) and torch.equal(rag[2], rag[3])


@pytest.mark.parametrize("kv", KV)
@pytest.mark.parametrize("model", MODELS)
def test_rewind_after_a_rejected_block(model, kv):
    """Session A runs a block of which two tokens are kept, rewinds and runs a second block; session B
    runs the two kept tokens alone, as one step, and the second block.  The rejected KV slots are
    overwritten and the rows of a step are computed independently, so the second block's logits are
    equal bit for bit.

    What couples rows, measured on an MI355X: the decode GEMMs.  The kernel table picks a kernel form
    per row-count bucket (up to 4, 16, 32, 48, 64 rows), and two forms do not add a row's products in the
    same order, so a row's last bits can depend on how many rows its step has.  On random inputs the
    small-llama lm_head GEMM's last row differs between a 1-row launch and a 5-row launch in 1 of 20
    draws and a 16-row launch in 2 of 20 (2, 3 and 8 rows: 0 of 20; tiny-llama: 0 of 20 at every
    count).  Through the KV cache that reaches this test when A's first block and B's step fall into
    different buckets: a 5-row block against B's 2-row step gave max |a - b| 0.0078 on small-llama
    bf16 (0.0 on tiny-llama and on both fp8 caches, whose e4m3 rounding absorbs it), and a one-token
    step for a single kept token (the decode path) 0.0098 / 0.0059 on the two models.  Both steps here
    have at most 4 rows, one bucket, which leaves the rewind itself as the only thing under test."""
    cfg, w, ex = _ex(model, kv)
    ids = _ids(cfg, 80, seed=1)
    P = 60
    ex.forward([("a", P), ("b", P)], torch.cat([ids[:P], ids[:P]]))
    block1 = torch.cat([ids[P:P + 2], _ids(cfg, 2, seed=2)])   # two kept tokens, then two rejected drafts
    block2 = ids[P + 2:P + 7]                                  # positions 62..66: across the page boundary
    ex.forward([("a", 4)], block1, logit_rows=[4])
    assert ex.sessions.get("a").length == P + 4
    a = ex.forward([("a", 5)], block2, starts=[P + 2], logit_rows=[5])
    assert ex.sessions.get("a").length == P + 7
    ex.forward([("b", 2)], ids[P:P + 2])
    b = ex.forward([("b", 5)], block2, logit_rows=[5])
    diff = float((a.float() - b.float()).abs().max())
    print(f"{model} kv={kv}: max |a - b| {diff}")
    assert torch.equal(a, b), diff


@pytest.mark.parametrize("kv", KV)
@pytest.mark.parametrize("model", MODELS)
def test_greedy_blocks_end_to_end(model, kv):
    """Executor + BatchSampler.verify with an oracle drafter that replays the plain greedy run, wrong
    on purpose at the third draft of every second block."""
    cfg, w, ex = _ex(model, kv)
    sampler = BatchSampler("cuda")
    greedy = SamplingParams(0.0, 1.0, 0, 1.0)
    ids = _ids(cfg, 20, seed=4)
    N, K = 16, 4
    t = int(torch.argmax(ex.forward([("p", 20)], ids).float(), -1))
    plain = [t]
    for _ in range(N - 1):
        t = int(torch.argmax(ex.forward([("p", 1)], torch.tensor([t], device="cuda")).float(), -1))
        plain.append(t)
    first = int(torch.argmax(ex.forward([("s", 20)], ids).float(), -1))
    assert first == plain[0]
    out, cur, block = [first], 21, 0
    while len(out) < N:
        d = plain[len(out):len(out) + K]
        wrong = block % 2 == 1 and len(d) > 2
        if wrong:
            d[2] = (d[2] + 1) % cfg.vocab_size
        x = torch.tensor([out[-1]] + d, device="cuda")
        logits = ex.forward([("s", len(d) + 1)], x, starts=[cur - 1], logit_rows=[len(d) + 1])
        kept = sampler.verify(logits, [d], [greedy], [out], [[7 + j for j in range(len(d) + 1)]])[0]
        am = logits.float().cpu().numpy().argmax(-1).tolist()  # per-position argmax of the step's own logits
        n = 0
        while n < len(d) and am[n] == d[n]:
            n += 1
        assert kept == am[:n + 1]
        assert len(kept) == (3 if wrong else len(d) + 1), (block, kept, d, am)
        out += kept
        cur += len(kept)
        block += 1
    assert out[:N] == plain
