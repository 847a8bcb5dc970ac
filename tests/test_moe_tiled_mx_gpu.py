"""Tiled grouped W8A8-MX MoE kernels (ops/csrc/gemm_moe_tiled_mx.hip) on the GPU: the slot-order quantizer
byte for byte against ops.quant_mx_rows of the slot-order matrix; gate/up and down + combine against an fp64
reference over ops.mx_block_quant of the gathered rows and the dequantized weights, at the bound
tests/test_mx_rows_gpu.py holds the dense MX GEMM to; run-to-run bit equality; unrouted experts never read; and
the fp8 Mixtral executor's switch MPAMD_MOE_TILED_MX.  CPU forms: tests/test_moe_tiled_mx.py.
"""
import pytest
import torch

from src import ops
from src.ops.reference import GU_BLOCK
from src.runtime.executor import StageExecutor

from .test_moe_fp8_gpu import _fp8_mixtral, expert_weights, rows
from .test_moe_rows_gpu import by_argsort, check, routing
from .test_moe_tiled import edge_routing

pytestmark = pytest.mark.gpu
DEV = "cuda"
SHAPES = [(256, 256, 4), (384, 1152, 4), (256, 14336, 8)]
ROUTINGS = [("pair", 65), ("skew", 257), ("random", 130), ("edge", 258)]
MX_ROUTE_FIGURE = 0.0093  # fp32 emulation (docstring of the executor test)
MX_ROUTE_BOUND = 2 * MX_ROUTE_FIGURE


def route(kind, T, E):
    return edge_routing(T, DEV) if kind == "edge" else routing(T, E, kind)


def run(x, act_in, weights, idx, w, E):
    gu8, gus, dn8, dns = weights
    off, tok, wsel = ops.moe_group(idx, w, E)
    return (ops.moe_gate_up_mx_tiled(x, gu8, gus, off, tok),
            ops.moe_down_mx_tiled(act_in, dn8, dns, off, tok, wsel, idx, x.shape[0]))


@pytest.mark.parametrize("kind,T", [("edge", 258), ("pair", 65)])
@pytest.mark.parametrize("H", [256, 384])
def test_quantizer_equals_quant_mx_rows_of_the_slot_order_matrix(H, kind, T):
    """Per live slot: its gathered rows, then zero rows up to 128.  Both forms, every byte of the live slots."""
    E = 4
    idx, w = route(kind, T, E)
    off, tok, _ = by_argsort(idx, w, E)
    o = off.tolist()
    if kind == "edge":
        assert o == [0, 128, 257, 258, 516]
    x = rows(T, H, 1)
    gathered = x[tok.long()]
    slots = []
    for e in range(E):
        for p0 in range(o[e], o[e + 1], 128):
            blk = torch.zeros(128, H, dtype=torch.bfloat16, device=DEV)
            blk[:min(128, o[e + 1] - p0)] = gathered[p0:min(p0 + 128, o[e + 1])]
            slots.append(blk)
    live = len(slots)
    for form in ((x, off, tok), (gathered, off)):
        got_ax, got_as = ops.moe_quant_mx_tiled(*form)
        want_ax, want_as = ops.quant_mx_rows(torch.cat(slots))
        assert got_ax.shape == (2 * T // 128 + E, 8, H // 128, 2, 64, 16) and got_as.shape[1:] == (2, H // 128, 64, 4)
        assert torch.equal(got_ax[:live].reshape(-1), want_ax.reshape(-1))
        assert torch.equal(got_as[:live].reshape(-1), want_as.reshape(-1))


@pytest.mark.parametrize("kind,T", ROUTINGS)
@pytest.mark.parametrize("H,F,E", SHAPES)
def test_gate_up_and_down_match_the_fp64_reference_and_repeat_bit_for_bit(H, F, E, kind, T):
    assert ops.moe_tiled_ok(T, E, 2, H, F)
    gu8, gus, dn8, dns = expert_weights(H, F, E)
    idx, w = route(kind, T, E)
    off, tok, wsel = by_argsort(idx, w, E)
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
        gu = ops.mx_block_quant(x[tok[sl].long()].float()).double() @ ops.unpack_weight_w8(gu8[e], gus[e], torch.float64).t()
        g, u = gu.view(-1, F // GU_BLOCK, 2, GU_BLOCK).unbind(2)
        want_act[sl] = (g * torch.sigmoid(g) * u).reshape(-1, F)
        ye = ops.mx_block_quant(act_in[sl].float()).double() @ ops.unpack_weight_w8(dn8[e], dns[e], torch.float64).t()
        want_y.index_add_(0, tok[sl].long(), ye * wsel[sl, None].double())
    check(act, want_act, f"gate/up H={H} F={F} E={E} T={T} {kind}")
    check(y, want_y, f"down H={H} F={F} E={E} T={T} {kind}")
    again = run(x, act_in, (gu8, gus, dn8, dns), idx, w, E)
    assert torch.equal(again[0], act) and torch.equal(again[1], y)


def test_unrouted_experts_are_never_read():
    """e4m3 NaN codes over the weights of every expert without a row."""
    H, F, E, T = 256, 14336, 8, 65
    gu8, gus, dn8, dns = expert_weights(H, F, E)
    idx, w = route("pair", T, E)
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


@pytest.mark.parametrize("env,mx,w8", [({"MPAMD_MOE_TILED": "65"}, False, True),
                                       ({"MPAMD_MOE_TILED_MX": "1"}, False, False),
                                       ({"MPAMD_MOE_TILED": "65", "MPAMD_MOE_TILED_MX": "1"}, True, False)])
def test_fp8_mixtral_prefill_runs_the_mx_ops_under_both_switches_only(env, mx, w8, monkeypatch):
    """An 80 + 9-token prefill.  With MPAMD_MOE_TILED=65 and MPAMD_MOE_TILED_MX=1 it runs the MX ops once per
    layer and the W8A16 tiled ones not at all; with MPAMD_MOE_TILED alone the reverse; the MX switch alone
    changes nothing.

    Bound on the relative Frobenius distance of the MX logits to the logits with every switch unset: an fp32
    torch run on the CPU over the same dequantized weights and prompts, once with ops.mx_block_quant on the two
    expert GEMM inputs of every layer and once without, puts the two sets of last-token logits 0.0093 apart
    (0.0105 for the 80-token prompt alone, 0.0080 for the 9-token one); the bound is twice that, 0.0186 (bf16
    intermediates and summation order, which the emulation does not have)."""
    cfg, mk, _ = _fp8_mixtral()
    calls = dict.fromkeys(("moe_gate_up_mx_tiled", "moe_down_mx_tiled", "moe_gate_up_w8_tiled", "moe_down_w8_tiled"), 0)
    for name in calls:
        def counted(*a, _f=getattr(ops, name), _n=name, **kw):
            calls[_n] += 1
            return _f(*a, **kw)

        monkeypatch.setattr(ops, name, counted)
    g = torch.Generator().manual_seed(3)
    ids = torch.cat([torch.randint(0, cfg.vocab_size, (n,), generator=g) for n in (80, 9)]).cuda()
    logits = {}
    for on in (False, True):
        for k in ("MPAMD_MOE_TILED", "MPAMD_MOE_TILED_MX"):
            monkeypatch.delenv(k, raising=False)
            if on and k in env:
                monkeypatch.setenv(k, env[k])
        ex = StageExecutor(cfg, mk(quant_type="fp8"), DEV, kv_cache_bytes=128 << 20, max_sessions=80, max_seq_len=128,
                           use_graphs=True, warmup=False)
        logits[on] = ex.forward([("a", 80), ("b", 9)], ids).float().clone()
        if not on:
            assert not any(calls.values())
    layers = cfg.num_hidden_layers
    assert (calls["moe_gate_up_mx_tiled"], calls["moe_down_mx_tiled"]) == ((layers, layers) if mx else (0, 0))
    assert (calls["moe_gate_up_w8_tiled"], calls["moe_down_w8_tiled"]) == ((layers, layers) if w8 else (0, 0))
    if not (mx or w8):
        assert torch.equal(logits[True], logits[False])
    if mx:
        assert bool(torch.isfinite(logits[True]).all())
        rel = float((logits[True] - logits[False]).norm() / logits[False].norm())
        print(f"MX tiled route vs every switch unset: rel fro {rel:.4g} (bound {MX_ROUTE_BOUND:.4g})")
        assert rel < MX_ROUTE_BOUND
