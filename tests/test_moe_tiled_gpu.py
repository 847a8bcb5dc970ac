"""Tiled grouped W8A16 MoE kernels (ops/csrc/gemm_moe_tiled.hip) on the GPU: gate/up and down + combine
against an fp64 reference over the dequantized weights at the project's W8A16 bound, on routings chosen for
the 128-row block edges; unrouted experts never read; run-to-run bit equality; the shape gate; and the fp8
Mixtral executor's switch MPAMD_MOE_TILED.  CPU forms: tests/test_moe_tiled.py.
"""
import pytest
import torch

from src import ops
from src.models.reference_model import reference_forward
from src.ops.reference import GU_BLOCK
from src.runtime.executor import StageExecutor

from .test_moe_fp8_gpu import _fp8_mixtral, expert_weights, rows
from .test_moe_rows_gpu import by_argsort, check, routing
from .test_moe_tiled import edge_routing

pytestmark = pytest.mark.gpu
DEV = "cuda"
SHAPES = [(256, 256, 4), (1152, 1152, 4), (256, 14336, 8)]
ROUTINGS = [("pair", 65), ("skew", 257), ("random", 130), ("edge", 258)]


def route(kind, T, E):
    return edge_routing(T, DEV) if kind == "edge" else routing(T, E, kind)


def run(x, act_in, weights, idx, w, E):
    gu8, gus, dn8, dns = weights
    off, tok, wsel = ops.moe_group(idx, w, E)
    return (ops.moe_gate_up_w8_tiled(x, gu8, gus, off, tok),
            ops.moe_down_w8_tiled(act_in, dn8, dns, off, tok, wsel, idx, x.shape[0]))


@pytest.mark.parametrize("kind,T", ROUTINGS)
@pytest.mark.parametrize("H,F,E", SHAPES)
def test_gate_up_and_down_match_the_fp64_reference_and_repeat_bit_for_bit(H, F, E, kind, T):
    assert ops.moe_tiled_ok(T, E, 2, H, F)
    gu8, gus, dn8, dns = expert_weights(H, F, E)
    idx, w = route(kind, T, E)
    off, tok, wsel = by_argsort(idx, w, E)
    if kind == "edge":
        assert off.tolist()[:5] == [0, 128, 257, 258, 516]
    x, act_in = rows(T, H, 1), rows(2 * T, F, 2)
    act, y = run(x, act_in, (gu8, gus, dn8, dns), idx, w, E)
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
    again = run(x, act_in, (gu8, gus, dn8, dns), idx, w, E)
    assert torch.equal(again[0], act) and torch.equal(again[1], y)


@pytest.mark.parametrize("kind,T", [("pair", 65), ("edge", 258)])
def test_unrouted_experts_are_never_read(kind, T):
    """e4m3 NaN codes over the weights of every expert without a row."""
    H, F, E = 256, 14336, 8
    gu8, gus, dn8, dns = expert_weights(H, F, E)
    idx, w = route(kind, T, E)
    x, act_in = rows(T, H, 1), rows(2 * T, F, 2)
    act, y = run(x, act_in, (gu8, gus, dn8, dns), idx, w, E)
    gu8n, dn8n = gu8.clone(), dn8.clone()
    unrouted = [e for e in range(E) if not bool((idx == e).any())]
    assert unrouted
    for e in unrouted:
        gu8n[e] = 0x7F
        dn8n[e] = 0x7F
    act2, y2 = run(x, act_in, (gu8n, gus, dn8n, dns), idx, w, E)
    assert torch.isfinite(act2.float()).all() and torch.equal(act2, act)
    assert torch.isfinite(y2.float()).all() and torch.equal(y2, y)


def test_uncovered_shapes_and_bad_arguments_launch_nothing():
    assert ops.moe_tiled_ok(65, 4, 2, 256, 256) and ops.moe_tiled_ok(8192, 8, 2, 4096, 14336)
    assert not ops.moe_tiled_ok(64, 4, 2, 256, 256) and not ops.moe_tiled_ok(65, 33, 2, 256, 256)
    assert not ops.moe_tiled_ok(65, 4, 2, 256, 96)
    gu8, gus, dn8, dns = expert_weights(256, 256, 4)
    idx, w = routing(65, 4, "random")
    off, tok, wsel = ops.moe_group(idx, w, 4)
    x = rows(65, 256, 1)
    out = torch.empty(130, 256, dtype=torch.bfloat16, device=DEV)
    ws = torch.empty(130 * 256, device=DEV)
    with pytest.raises(RuntimeError, match="off"):
        torch.ops.mpamd.moe_gate_up_w8_tiled(x, gu8, gus, off.long(), tok, out)
    with pytest.raises(RuntimeError, match="idx"):
        torch.ops.mpamd.moe_down_w8_tiled(out, dn8, dns, off, tok, wsel, idx.int(), ws)
    with pytest.raises(RuntimeError, match="ws"):
        torch.ops.mpamd.moe_combine_tiled(ws.double(), idx, torch.empty(65, 256, dtype=torch.bfloat16, device=DEV), 4)
    with pytest.raises(ValueError, match="idx"):
        ops.moe_down_w8_tiled(out, dn8, dns, off, tok, wsel, idx.int(), 65)
    torch.cuda.synchronize()


# ------------------------------------------------------------------ executor
def _count(monkeypatch):
    calls = {}
    for name in ("moe_gate_up_w8_tiled", "moe_down_w8_tiled", "moe_gate_up_w8_rows", "moe_down_w8_rows"):
        calls[name] = 0

        def counted(*a, _f=getattr(ops, name), _n=name, **kw):
            calls[_n] += 1
            return _f(*a, **kw)

        monkeypatch.setattr(ops, name, counted)
    return calls


@pytest.mark.parametrize("env,prefill,decode", [({"MPAMD_MOE_TILED": "65"}, True, False), ({}, False, False),
                                                ({"MPAMD_MOE_TILED": "65", "MPAMD_MOE_ROWS_DECODE": "1"}, True, True)])
def test_fp8_mixtral_steps_run_the_tiled_ops_under_the_switch_only(env, prefill, decode, monkeypatch):
    """An 80 + 9-token prefill and a 65-session decode step against the fp32 oracle over the dequantized weights
    (test_fp8_mixtral_executor's bound).  With MPAMD_MOE_TILED=65 the prefill runs the tiled ops once per layer
    and the row-gathered ones not at all; a pure decode step follows only with MPAMD_MOE_ROWS_DECODE=1; with
    the switch unset no step takes them."""
    cfg, mk, oracle = _fp8_mixtral()
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    calls = _count(monkeypatch)
    ex = StageExecutor(cfg, mk(quant_type="fp8"), DEV, kv_cache_bytes=128 << 20, max_sessions=80, max_seq_len=128,
                       use_graphs=True, warmup=False)
    layers = cfg.num_hidden_layers
    tiled = lambda: (calls["moe_gate_up_w8_tiled"], calls["moe_down_w8_tiled"])  # noqa: E731
    g = torch.Generator().manual_seed(3)
    prompts = [torch.randint(0, cfg.vocab_size, (n,), generator=g) for n in (80, 9)]
    logits = ex.forward([("a", 80), ("b", 9)], torch.cat(prompts).cuda())
    assert tiled() == ((layers, layers) if prefill else (0, 0))
    if prefill:
        assert calls["moe_gate_up_w8_rows"] == calls["moe_down_w8_rows"] == 0
    for i, p in enumerate(prompts):
        torch.testing.assert_close(logits[i].float(), reference_forward([oracle], p.cuda())[-1], atol=0.06, rtol=0.05)
    n, plen = 65, 3
    ids = torch.randint(0, cfg.vocab_size, (n, plen), generator=g)
    nxt = torch.argmax(ex.forward([(f"s{i}", plen) for i in range(n)], ids.reshape(-1).cuda()).float(), -1)
    before = tiled()
    logits = ex.forward([(f"s{i}", 1) for i in range(n)], nxt)
    assert tiled() == tuple(b + (layers if decode else 0) for b in before)
    for i in (0, 64):
        seq = torch.cat([ids[i], nxt[i:i + 1].cpu()]).cuda()
        torch.testing.assert_close(logits[i].float(), reference_forward([oracle], seq)[-1], atol=0.06, rtol=0.05)
