"""The batched LoRA kernels (csrc/lora.hip) and the executor's LoRA steps on the GPU.

Kernel shapes (K, N, R): the smallest and the largest of each dimension and an odd middle - K 128 (fewer
8-column pieces than lanes), 384, 4096; N 16 (two active threads), 528 (a partial workgroup), 12288 (twelve
workgroups per row); R 16, 48, 192 (the limit).  Rows: one, a partial tile, a full tile, a tile + 1,
three-and-a-bit tiles, all four.  S = 4 adapters; the stacks are made once per shape.

Bounds (derived, not measured): bf16 x bf16 products are exact in fp32, so only the accumulation rounds.
  shrink:  |t - t64| <= 2 K 2^-24 scale sum_k |A x|_k
  expand, given the kernel's own fp32 t:
           |y' - y64| <= 2^-8 |y64| + 2 (R + 2) 2^-24 (|y| + sum_j |B t|_j)
(the factor 2 is slack for fused versus unfused multiply-add; 2^-8 is the final bf16 rounding).
"""
import functools

import pytest
import torch

from src import ops
from src.models.adapters import merged_weights
from src.models.config import resolve_model
from src.models.reference_model import reference_forward
from src.models.weights import random_stage_weights
from src.runtime.executor import StageExecutor

pytestmark = pytest.mark.gpu
DEV = "cuda"
S = 4
SHAPES = [(128, 16, 16), (384, 528, 48), (4096, 12288, 192), (4096, 16, 48), (128, 12288, 16), (384, 528, 192)]
MS = [1, 13, 16, 17, 50, 64]
PATTERNS = ["one", "none", "mixed", "cyclic"]
NAN = float("nan")


@functools.lru_cache(maxsize=None)
def stacks(K, N, R):
    """(A [S, R, K], B [S, N, R], scale [S]): entries ~ N(0, 1) / sqrt(inner dimension)."""
    g = torch.Generator(device=DEV).manual_seed(K * 31 + N * 7 + R)
    A = (torch.randn(S, R, K, device=DEV, generator=g) * K ** -0.5).to(torch.bfloat16)
    B = (torch.randn(S, N, R, device=DEV, generator=g) * R ** -0.5).to(torch.bfloat16)
    return A, B, torch.tensor([2.0, 0.5, 1.0, 16 / 8 ** 0.5], device=DEV)


def slots_of(M, pattern):
    if pattern == "one":
        sl = torch.full((M,), 2)
    elif pattern == "none":
        sl = torch.full((M,), -1)
    elif pattern == "cyclic":  # every row of a tile a different slot than its neighbours
        sl = torch.arange(M) % S
    else:  # adapters 0, 1, 3 and base rows; slot 2 unused
        sl = torch.tensor([(0, -1, 3, 1, -1)[(m * 7 + m // 5) % 5] for m in range(M)])
    return sl.to(torch.int32).to(DEV)


def rows(M, K, seed):
    g = torch.Generator(device=DEV).manual_seed(seed)
    return torch.randn(M, K, device=DEV, generator=g).to(torch.bfloat16)


def pack_padded(x, pad):
    """Packed activation of x's rows with the padding rows of the last 16-row tile set to ``pad``."""
    M, K = x.shape
    full = torch.full((((M + 15) // 16) * 16, K), pad, dtype=x.dtype, device=x.device)
    full[:M] = x
    return ops.pack_act(full)


def poisoned(A, B, sl):
    """Copies of the stacks with NaN in every slot no row names."""
    used = set(int(s) for s in sl.tolist() if s >= 0)
    A, B = A.clone(), B.clone()
    for s in range(S):
        if s not in used:
            A[s] = NAN
            B[s] = NAN
    return A, B


def run_pair(M, K, N, R, sl, y0, x):
    """shrink + expand with everything a LoRA op must not read set to NaN -> (t, y)."""
    A, B, scale = stacks(K, N, R)
    Ap, Bp = poisoned(A, B, sl)
    base = sl < 0
    xq = x.clone()
    xq[base] = NAN
    t = torch.full((M, R), NAN, dtype=torch.float32, device=DEV)
    ops.lora_shrink(pack_padded(xq, NAN), Ap, scale, sl, M, out=t)
    y = y0.clone()
    ops.lora_expand(t, Bp, sl, y)
    return t, y


@pytest.mark.parametrize("pattern", PATTERNS)
@pytest.mark.parametrize("M", MS)
@pytest.mark.parametrize("K,N,R", SHAPES)
def test_kernels_within_the_derived_bounds_and_read_only_their_rows(K, N, R, M, pattern):
    assert ops.lora_ok(M, N, K, R)
    A, B, scale = stacks(K, N, R)
    sl = slots_of(M, pattern)
    x, y0 = rows(M, K, 1), rows(M, N, 2)
    t, y = run_pair(M, K, N, R, sl, y0, x)
    live = sl >= 0
    # base rows: t not written (still the NaN fill), y bit-unchanged
    assert bool(torch.isnan(t[~live]).all())
    assert torch.equal(y[~live], y0[~live])
    if pattern == "none":
        assert torch.equal(y, y0)
        return
    idx, s = torch.nonzero(live).flatten(), sl[live].long()
    assert not bool(torch.isnan(t[idx]).any()) and not bool(torch.isnan(y[idx].float()).any())
    # shrink against fp64
    prod = A[s].double() * x[idx].double()[:, None, :]                  # [m, R, K] exact products
    sc = scale[s].double()[:, None]
    t64 = sc * prod.sum(-1)
    bound = 2 * K * 2.0 ** -24 * sc * prod.abs().sum(-1)
    exc = ((t[idx].double() - t64).abs() - bound).max().item()
    print(f"LORA_SHRINK K={K} R={R} M={M} {pattern}: max err {(t[idx].double() - t64).abs().max().item():.3e} "
          f"worst err - bound {exc:.3e}")
    assert exc <= 0
    # expand against fp64, given the kernel's own t
    bt = B[s].double() * t[idx].double()[:, None, :]                     # [m, N, R]
    y64 = y0[idx].double() + bt.sum(-1)
    bound = 2.0 ** -8 * y64.abs() + 2 * (R + 2) * 2.0 ** -24 * (y0[idx].double().abs() + bt.abs().sum(-1))
    exc = ((y[idx].double() - y64).abs() - bound).max().item()
    print(f"LORA_EXPAND N={N} R={R} M={M} {pattern}: max err {(y[idx].double() - y64).abs().max().item():.3e} "
          f"worst err - bound {exc:.3e}")
    assert exc <= 0


@pytest.mark.parametrize("K,N,R", [(384, 528, 48), (4096, 12288, 192)])
def test_a_row_does_not_depend_on_the_other_rows_slots(K, N, R):
    M, m = 50, 19
    x, y0 = rows(M, K, 3), rows(M, N, 4)
    got = []
    for other in ("cyclic", "mixed", "none"):
        sl = slots_of(M, other)
        sl[m] = 1
        t, y = run_pair(M, K, N, R, sl, y0, x)
        got.append((t[m].clone(), y[m].clone()))
    for t, y in got[1:]:
        assert torch.equal(t, got[0][0]) and torch.equal(y, got[0][1])


def test_uncovered_shapes_and_bad_arguments():
    for M, N, K, R in ((65, 16, 128, 16), (4, 16, 100, 16), (4, 20, 128, 16), (4, 16, 128, 24), (4, 16, 128, 208)):
        assert not ops.lora_ok(M, N, K, R), (M, N, K, R)
    assert not ops.lora_ok(0, 16, 128, 16) and ops.lora_ok(64, 16, 128, 192)
    sl = torch.zeros(4, dtype=torch.int32, device=DEV)
    scale = torch.ones(S, device=DEV)
    # not covered: nothing written, the op says so
    A = torch.ones(S, 24, 128, dtype=torch.bfloat16, device=DEV)
    t = torch.full((4, 24), 7.0, device=DEV)
    with pytest.raises(RuntimeError, match="no kernel covers"):
        ops.lora_shrink(ops.pack_act(rows(4, 128, 5)), A, scale, sl, 4, out=t)
    B = torch.ones(S, 20, 16, dtype=torch.bfloat16, device=DEV)
    y = torch.full((4, 24), 7.0, dtype=torch.bfloat16, device=DEV)[:, :20]
    with pytest.raises(RuntimeError, match="no kernel covers"):
        ops.lora_expand(torch.ones(4, 16, device=DEV), B, sl, y)
    torch.cuda.synchronize()
    assert bool((t == 7.0).all()) and bool((y == 7.0).all())
    # M == 0 launches nothing
    A, B, scale = stacks(128, 16, 16)
    ops.lora_shrink(ops.pack_act(rows(1, 128, 5)), A, scale, sl, 0, out=torch.zeros(0, 16, device=DEV))
    # bad calls
    x = ops.pack_act(rows(4, 128, 5))
    with pytest.raises(ValueError, match="slots"):
        ops.lora_shrink(x, A, scale, sl.long(), 4)
    with pytest.raises(ValueError, match="slots"):
        ops.lora_shrink(x, A, scale, sl[:2], 4)
    with pytest.raises(ValueError, match="t must be"):
        ops.lora_shrink(x, A, scale, sl, 4, out=torch.zeros(4, 32, device=DEV))
    with pytest.raises(ValueError, match="scale"):
        ops.lora_shrink(x, A, scale[:2], sl, 4)
    with pytest.raises(ValueError, match="packed x"):
        ops.lora_shrink(x[:64], A, scale, sl, 4)
    with pytest.raises(ValueError, match="y must be"):
        ops.lora_expand(torch.zeros(4, 16, device=DEV), B, sl, torch.zeros(4, 24, dtype=torch.bfloat16, device=DEV))
    with pytest.raises(RuntimeError):  # the binding's own checks: fp32 where bf16 is due
        torch.ops.mpamd.lora_shrink(x, A.float(), scale, sl, torch.zeros(4, 16, device=DEV), 4)


# ------------------------------------------------------------------------------------------- executor
ALL7 = "q_proj,k_proj,v_proj,o_proj,gate_proj,up_proj,down_proj"
SPECS = ["synthetic:qv:16", f"synthetic:all:8:{ALL7}"]
PROMPTS = (37, 5)
KW = dict(kv_cache_bytes=256 << 20, max_sessions=80, max_seq_len=512)


@functools.lru_cache(maxsize=None)
def stage(model, adapters=True):
    cfg = resolve_model(model)
    w = random_stage_weights(cfg, 0, cfg.num_hidden_layers, has_embed=True, has_head=True, device=DEV,
                             dtype=torch.bfloat16, seed=3)
    if adapters:
        w.load_adapters(SPECS)
    return cfg, w


@functools.lru_cache(maxsize=None)
def oracle_weights(model, slot):
    return merged_weights(stage(model)[1], slot)


def oracle_error(model, ex, name, steps=4):
    """Max |logit - oracle| of sessions on adapter ``name`` over a ragged prefill and ``steps`` decode steps."""
    cfg, _ = stage(model)
    wf = [oracle_weights(model, ex.adapter_slot(name))]
    g = torch.Generator().manual_seed(0)
    seqs = [torch.randint(0, cfg.vocab_size, (n,), generator=g).to(DEV) for n in PROMPTS]
    sids = [f"{name}/{i}" for i in range(len(seqs))]
    ad = [name] * len(seqs)
    logits = ex.forward(list(zip(sids, PROMPTS)), torch.cat(seqs), adapters=ad)
    err = 0.0
    for _ in range(steps + 1):
        for i, p in enumerate(seqs):
            err = max(err, (logits[i].float() - reference_forward(wf, p)[-1]).abs().max().item())
        nxt = torch.argmax(logits.float(), -1)
        seqs = [torch.cat([s, nxt[i:i + 1]]) for i, s in enumerate(seqs)]
        logits = ex.forward([(s, 1) for s in sids], nxt, adapters=ad)
    return err


@pytest.mark.parametrize("model", ["small-llama", "tiny-llama"])
def test_lora_runs_stay_within_twice_the_base_models_own_error(model):
    cfg, w = stage(model)
    ex = StageExecutor(cfg, w, DEV, **KW)
    base = oracle_error(model, ex, "")
    assert ex.last_graphed and not ex._lora_graphs
    for name in ("qv", "all"):
        err = oracle_error(model, ex, name)
        assert ex.last_graphed and ex._lora_graphs
        print(f"LORA_ORACLE {model} {name}: max logit error {err:.4f} vs base {base:.4f} (ratio {err / base:.2f})")
        assert err <= 2 * base, (name, err, base)


def decode_run(ex, names, steps=3, tag=""):
    """Ragged prefill (5 + i tokens) then ``steps`` decode steps of one session per name -> logits per step."""
    cfg = ex.cfg
    sids = [f"{tag}s{i}" for i in range(len(names))]
    lens = [5 + i % 7 for i in range(len(names))]
    ids = torch.cat([(torch.arange(n, device=DEV) * (3 + i) + i) % cfg.vocab_size for i, n in enumerate(lens)])
    out = [ex.forward(list(zip(sids, lens)), ids, adapters=names).clone()]
    for _ in range(steps):  # (a replay returns a view of the graph's static output: copied before the next one)
        out.append(ex.forward([(s, 1) for s in sids], torch.argmax(out[-1].float(), -1), adapters=names).clone())
    return out


def test_mixed_batch_equals_each_session_alone():
    cfg, w = stage("small-llama")
    names = ["qv", "all", ""]
    both = decode_run(StageExecutor(cfg, w, DEV, **KW), names)
    for i, name in enumerate(names):
        ex = StageExecutor(cfg, w, DEV, **KW)
        # the same prompt and the same forced tokens as session i of the batch
        sid, n = "solo", 5 + i
        ids = (torch.arange(n, device=DEV) * (3 + i) + i) % cfg.vocab_size
        lg = ex.forward([(sid, n)], ids, adapters=[name])
        for step in range(1, len(both)):
            torch.testing.assert_close(lg[0].float(), both[step - 1][i].float(), atol=2e-2, rtol=2e-2)
            lg = ex.forward([(sid, 1)], torch.argmax(both[step - 1][i:i + 1].float(), -1), adapters=[name]).clone()
        torch.testing.assert_close(lg[0].float(), both[-1][i].float(), atol=2e-2, rtol=2e-2)


def test_base_steps_on_an_adapter_stage_equal_a_stage_without_adapters():
    cfg, w = stage("small-llama")
    _, w0 = stage("small-llama", adapters=False)
    a, b = StageExecutor(cfg, w, DEV, **KW), StageExecutor(cfg, w0, DEV, **KW)
    ra, rb = decode_run(a, ["", "", ""]), decode_run(b, ["", "", ""])
    assert a.last_graphed and b.last_graphed and not a._lora_graphs
    assert a._graphs.keys() == b._graphs.keys()
    for x, y in zip(ra, rb):
        assert torch.equal(x, y)


def test_lora_graphs_equal_eager_and_read_the_slots_at_replay():
    cfg, w = stage("small-llama")
    eager, graph = StageExecutor(cfg, w, DEV, use_graphs=False, **KW), StageExecutor(cfg, w, DEV, use_graphs=True, **KW)
    for k, names in enumerate((["qv", "all", "", "qv"], ["", "qv", "qv", "all"], ["all", "", "all", ""])):
        re_, rg = decode_run(eager, names, tag=f"p{k}"), decode_run(graph, names, tag=f"p{k}")
        assert graph.last_graphed and not eager.last_graphed
        for x, y in zip(re_, rg):
            assert torch.equal(x, y), names
    # one captured graph served all three slot patterns: the slots are data of the replay
    assert len(graph._lora_graphs) == 1 and not graph._graphs
    graph.clear_graphs()
    assert not graph._lora_graphs


def test_a_65_row_lora_step_is_not_graphed_and_matches_the_oracle():
    model = "tiny-llama"
    cfg, w = stage(model)
    ex = StageExecutor(cfg, w, DEV, **KW)
    names = [("qv", "", "all")[i % 3] for i in range(65)]
    out = decode_run(ex, names, steps=1)
    assert not ex.last_graphed and not ex._lora_graphs
    ids = [(torch.arange(5 + i % 7, device=DEV) * (3 + i) + i) % cfg.vocab_size for i in range(65)]
    nxt = torch.argmax(out[0].float(), -1)
    for i in range(0, 65, 4):
        wf = [oracle_weights(model, ex.adapter_slot(names[i]))]
        torch.testing.assert_close(out[1][i].float(), reference_forward(wf, torch.cat([ids[i], nxt[i:i + 1]]))[-1],
                                   atol=0.06, rtol=0.05)
