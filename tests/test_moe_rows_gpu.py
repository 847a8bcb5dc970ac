"""Row-gathered grouped W8A16 MoE kernels (ops/csrc/gemm_moe_rows.hip) on the GPU: the device grouping
against the stable argsort, gate/up and down against an fp64 reference over the dequantized weights at
the project's W8A16 bound, unrouted experts never read, run-to-run bit equality, and the fp8 Mixtral
executor's steps above 64 rows (the switch MPAMD_MOE_ROWS included).  CPU forms: tests/test_moe_rows.py.
"""
import pytest
import torch

from src import ops
from src.models.reference_model import reference_forward
from src.ops import moe
from src.ops.reference import GU_BLOCK
from src.runtime.executor import StageExecutor

from .test_moe_fp8_gpu import _fp8_mixtral, expert_weights, rows

pytestmark = pytest.mark.gpu
DEV = "cuda"
SHAPES = [(256, 256, 4), (1152, 1152, 4), (256, 14336, 8), (4096, 256, 8)]
TS = [65, 130]
ROUTINGS = ["pair", "skew", "random"]


def routing(T, E, kind):
    """(idx int64 [T, 2], w fp32 [T, 2]) with known counts: "pair" every token to experts (1, 2);
    "skew" token t to (0, 1 + t % (E - 1)); "random" moe.route of seeded logits."""
    g = torch.Generator(device=DEV).manual_seed(T * 13 + E)
    logits = torch.randn(T, E, device=DEV, generator=g)
    if kind == "random":
        w, idx = moe.route(logits, 2)
        return idx, w
    t = torch.arange(T, device=DEV)
    idx = torch.stack([torch.ones_like(t), 2 * torch.ones_like(t)] if kind == "pair" else
                      [torch.zeros_like(t), 1 + t % (E - 1)], 1)
    w = torch.softmax(logits.gather(1, idx), -1)
    return idx, w


def by_argsort(idx, w, E):
    flat = idx.reshape(-1)
    order = torch.argsort(flat, stable=True)
    off = torch.zeros(E + 1, dtype=torch.int32, device=idx.device)
    off[1:] = torch.cumsum(torch.bincount(flat, minlength=E), 0)
    return off, (order // idx.shape[1]).to(torch.int32), w.reshape(-1)[order]


def check(got, want, what):
    """test_down_general_routing_matches_the_fp32_oracle's W8A16 bound, over every output row."""
    err = float((got.double() - want).norm() / want.norm())
    print(f"{what}: max abs err {float((got.double() - want).abs().max()):.4g}, rel fro {err:.3g}")
    torch.testing.assert_close(got.double(), want, atol=5e-2, rtol=2e-2)
    assert err < 1e-2


@pytest.mark.parametrize("kind", ROUTINGS)
@pytest.mark.parametrize("T", TS)
@pytest.mark.parametrize("E", [4, 8])
def test_group_equals_the_stable_argsort(E, T, kind):
    idx, w = routing(T, E, kind)
    off, tok, wsel = ops.moe_group(idx, w, E)
    want = by_argsort(idx, w, E)
    assert off.dtype == tok.dtype == torch.int32 and wsel.dtype == torch.float32
    for got, ref in zip((off, tok, wsel), want):
        assert torch.equal(got, ref)
    if kind == "pair":
        assert off.tolist() == [0, 0, T] + [2 * T] * (E - 2)


@pytest.mark.parametrize("kind", ROUTINGS)
@pytest.mark.parametrize("T", TS)
@pytest.mark.parametrize("H,F,E", SHAPES)
def test_gate_up_and_down_match_the_fp64_reference_and_repeat_bit_for_bit(H, F, E, T, kind):
    assert ops.moe_rows_ok(T, E, 2, H, F)
    gu8, gus, dn8, dns = expert_weights(H, F, E)
    idx, w = routing(T, E, kind)
    off, tok, wsel = by_argsort(idx, w, E)
    x, act_in = rows(T, H, 1), rows(2 * T, F, 2)
    act = ops.moe_gate_up_w8_rows(x, gu8, gus, off, tok)
    y = ops.moe_down_w8_rows(act_in, dn8, dns, off, tok, wsel, T)
    assert act.shape == (2 * T, F) and y.shape == (T, H) and act.dtype == y.dtype == torch.bfloat16
    want_act = torch.zeros(2 * T, F, dtype=torch.float64, device=DEV)
    want_y = torch.zeros(T, H, dtype=torch.float64, device=DEV)
    o = off.tolist()
    for e in range(E):
        sl = slice(o[e], o[e + 1])
        if o[e + 1] == o[e]:
            continue
        gu = x[tok[sl].long()].double() @ ops.unpack_weight_w8(gu8[e], gus[e], torch.float64).t()
        g, u = gu.view(-1, F // GU_BLOCK, 2, GU_BLOCK).unbind(2)
        want_act[sl] = (g * torch.sigmoid(g) * u).reshape(-1, F)
        ye = act_in[sl].double() @ ops.unpack_weight_w8(dn8[e], dns[e], torch.float64).t()
        want_y.index_add_(0, tok[sl].long(), ye * wsel[sl, None].double())
    check(act, want_act, f"gate/up H={H} F={F} E={E} T={T} {kind}")
    check(y, want_y, f"down H={H} F={F} E={E} T={T} {kind}")
    assert torch.equal(ops.moe_gate_up_w8_rows(x, gu8, gus, off, tok), act)
    assert torch.equal(ops.moe_down_w8_rows(act_in, dn8, dns, off, tok, wsel, T), y)


@pytest.mark.parametrize("T", TS)
@pytest.mark.parametrize("H,F,E", SHAPES)
def test_unrouted_experts_are_never_read(H, F, E, T):
    """e4m3 NaN codes over the weights of every expert but the routed 1 and 2."""
    gu8, gus, dn8, dns = expert_weights(H, F, E)
    off, tok, wsel = ops.moe_group(*routing(T, E, "pair"), E)
    x, act_in = rows(T, H, 1), rows(2 * T, F, 2)
    act = ops.moe_gate_up_w8_rows(x, gu8, gus, off, tok)
    y = ops.moe_down_w8_rows(act_in, dn8, dns, off, tok, wsel, T)
    gu8n, dn8n = gu8.clone(), dn8.clone()
    for e in [0] + list(range(3, E)):
        gu8n[e] = 0x7F
        dn8n[e] = 0x7F
    act2 = ops.moe_gate_up_w8_rows(x, gu8n, gus, off, tok)
    y2 = ops.moe_down_w8_rows(act_in, dn8n, dns, off, tok, wsel, T)
    assert torch.isfinite(act2.float()).all() and torch.equal(act2, act)
    assert torch.isfinite(y2.float()).all() and torch.equal(y2, y)


def test_uncovered_shapes_and_bad_arguments_launch_nothing():
    assert ops.moe_rows_ok(65, 4, 2, 256, 256)
    assert not ops.moe_rows_ok(65, 4, 2, 256, 96) and not ops.moe_rows_ok(65, 33, 2, 256, 256)
    assert not ops.moe_rows_ok(0, 4, 2, 256, 256)
    gu8, gus, dn8, dns = expert_weights(256, 256, 4)
    idx, w = routing(65, 4, "random")
    off, tok, wsel = ops.moe_group(idx, w, 4)
    x = rows(65, 256, 1)
    out = torch.empty(130, 256, dtype=torch.bfloat16, device=DEV)
    with pytest.raises(RuntimeError, match="idx"):
        torch.ops.mpamd.moe_group(idx.int(), w, off, tok, wsel)
    with pytest.raises(RuntimeError, match="off"):
        torch.ops.mpamd.moe_gate_up_w8_rows(x, gu8, gus, off.long(), tok, out)
    with pytest.raises(RuntimeError, match="out"):
        torch.ops.mpamd.moe_gate_up_w8_rows(x, gu8, gus, off, tok, out[:, :128])
    with pytest.raises(ValueError, match="wsel"):
        ops.moe_down_w8_rows(out, dn8, dns, off, tok, wsel.double(), 65)
    with pytest.raises(RuntimeError, match="ws"):
        torch.ops.mpamd.moe_down_w8_rows(out, dn8, dns, off, tok, wsel, torch.empty(16, device=DEV),
                                         torch.empty(65, 256, dtype=torch.bfloat16, device=DEV))
    torch.cuda.synchronize()


# ------------------------------------------------------------------ executor
def _count_rows_ops(monkeypatch):
    calls = {}
    for name in ("moe_group", "moe_gate_up_w8_rows", "moe_down_w8_rows"):
        calls[name] = 0

        def counted(*a, _f=getattr(ops, name), _n=name, **kw):
            calls[_n] += 1
            return _f(*a, **kw)

        monkeypatch.setattr(ops, name, counted)
    return calls


@pytest.mark.parametrize("env,prefill,decode", [({}, True, False), ({"MPAMD_MOE_ROWS_DECODE": "1"}, True, True),
                                                ({"MPAMD_MOE_ROWS": "0", "MPAMD_MOE_ROWS_DECODE": "1"}, False, False)])
def test_fp8_mixtral_steps_above_64_rows_run_the_row_gathered_ops(env, prefill, decode, monkeypatch):
    """An 80 + 9-token prefill and a 65-session decode step against the fp32 oracle over the dequantized
    weights (test_fp8_mixtral_executor's bound).  Prefill steps take the new ops by default; a pure decode
    step keeps the dequantizing schedule (its launches are a recorded trace, tests/golden/executor_paths)
    unless MPAMD_MOE_ROWS_DECODE=1; MPAMD_MOE_ROWS=0 keeps the dequantizing schedule everywhere."""
    cfg, mk, oracle = _fp8_mixtral()
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    calls = _count_rows_ops(monkeypatch)
    ex = StageExecutor(cfg, mk(quant_type="fp8"), DEV, kv_cache_bytes=128 << 20, max_sessions=80, max_seq_len=128,
                       use_graphs=True, warmup=False)
    layers = cfg.num_hidden_layers
    g = torch.Generator().manual_seed(3)
    prompts = [torch.randint(0, cfg.vocab_size, (n,), generator=g) for n in (80, 9)]
    logits = ex.forward([("a", 80), ("b", 9)], torch.cat(prompts).cuda())
    assert set(calls.values()) == {layers if prefill else 0}
    for i, p in enumerate(prompts):
        torch.testing.assert_close(logits[i].float(), reference_forward([oracle], p.cuda())[-1], atol=0.06, rtol=0.05)
    n, plen = 65, 3
    ids = torch.randint(0, cfg.vocab_size, (n, plen), generator=g)
    nxt = torch.argmax(ex.forward([(f"s{i}", plen) for i in range(n)], ids.reshape(-1).cuda()).float(), -1)
    before = dict(calls)
    logits = ex.forward([(f"s{i}", 1) for i in range(n)], nxt)
    assert all(calls[k] == before[k] + (layers if decode else 0) for k in calls)
    for i in (0, 64):
        seq = torch.cat([ids[i], nxt[i:i + 1].cpu()]).cuda()
        torch.testing.assert_close(logits[i].float(), reference_forward([oracle], seq)[-1], atol=0.06, rtol=0.05)
