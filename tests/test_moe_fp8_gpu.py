"""The grouped W8A16 MoE kernels (csrc/gemm_moe.hip) and the fp8 Mixtral executor path on the GPU.

Shapes (H, F, E): tiny-mixtral; 9 ring steps per wave (the clamped ring tail); gate/up 4 / 2 and down
2 / 1 tile widths; Mixtral's gate/up 8 / 6 widths; down on 256 workgroups.  Rows: one, a partial tile, a
full tile, a tile + 1, three-and-a-bit tiles, all four tiles.  Weights are made once per shape.
"""
import functools

import pytest
import torch

from src import ops
from src.models.config import resolve_model
from src.models.reference_model import reference_forward
from src.models.weights import random_stage_weights
from src.ops import moe
from src.runtime.executor import StageExecutor

from .test_moe_fp8 import dequantized

pytestmark = pytest.mark.gpu
DEV = "cuda"
SHAPES = [(256, 256, 4), (1152, 1152, 4), (256, 6144, 4), (6144, 256, 4), (256, 14336, 8), (4096, 256, 8)]
MS = [1, 13, 16, 17, 50, 64]
SENTINEL = 7.0


@functools.lru_cache(maxsize=None)
def expert_weights(H, F, E):
    """(gate_up w8 [E, 2F/16, H/32, 64, 8], scales [E, 2F], down w8, scales [E, H]); w ~ 0.02 N(0, 1)."""
    g = torch.Generator(device=DEV).manual_seed(H * 31 + F * 7 + E)

    def stack(N, K):
        q8, sc = [], []
        for _ in range(E):
            q, s = ops.pack_weight_fp8(0.02 * torch.randn(N, K, device=DEV, generator=g))
            q8.append(ops.w8_from_fp8(q))
            sc.append(s)
        return torch.stack(q8), torch.stack(sc)

    return stack(2 * F, H) + stack(H, F)


def routing(M, E, kind, seed=0):
    """Dense routing matrix fp32 [M, E] + counts: "all" top-2 over every expert, "edges" top-2 with the
    first and last expert unrouted, ("one", e) expert e alone with weight 1."""
    if isinstance(kind, tuple):
        wd = torch.zeros(M, E, device=DEV)
        wd[:, kind[1]] = 1.0
    else:
        g = torch.Generator(device=DEV).manual_seed(seed + M)
        logits = torch.randn(M, E, device=DEV, generator=g)
        if kind == "edges":
            logits[:, 0] = logits[:, E - 1] = -1e9
        wd = moe.dense_weights(*moe.route(logits, 2), E)
    return wd, (wd > 0).sum(0, dtype=torch.int32)


def rows(M, K, seed):
    g = torch.Generator(device=DEV).manual_seed(seed)
    return torch.randn(M, K, device=DEV, generator=g).to(torch.bfloat16)


def pack_padded(x, pad):
    """Packed activation of x's rows with the padding rows of the last 16-row tile set to ``pad``."""
    M, K = x.shape
    full = torch.full((((M + 15) // 16) * 16, K), pad, dtype=x.dtype, device=x.device)
    full[:M] = x
    return ops.pack_act(full)


def act_slabs(M, F, E, seed, pad=0.0):
    """E packed activations ~ N(0, 1) (the down kernel's input) + the row-major originals."""
    xs = [rows(M, F, seed + e) for e in range(E)]
    return torch.cat([pack_padded(x, pad) for x in xs]), xs


def down_oracle(xs, dn8, dns, wd):
    tot = torch.zeros(wd.shape[0], dn8.shape[1] * 16, dtype=torch.float32, device=DEV)
    for e in range(len(xs)):
        if bool((wd[:, e] > 0).any()):
            tot += wd[:, e:e + 1] * (xs[e].float() @ ops.unpack_weight_w8(dn8[e], dns[e], torch.float32).t())
    return tot


@pytest.mark.parametrize("kind", ["all", "edges"])
@pytest.mark.parametrize("M", MS)
@pytest.mark.parametrize("H,F,E", SHAPES)
def test_gate_up_slabs_equal_the_single_expert_gemm_bit_for_bit(H, F, E, M, kind, monkeypatch):
    assert ops.moe_w8_ok(M, E, H, F)
    monkeypatch.setattr(ops, "_W8_MODE", "rw")
    gu8, gus, _, _ = expert_weights(H, F, E)
    xp = ops.pack_act(rows(M, H, 1))
    _, cnt = routing(M, E, kind)
    slab = ops.packed_numel(M, F)
    act = torch.full((E * slab,), SENTINEL, dtype=torch.bfloat16, device=DEV)
    ops.moe_gate_up_w8(xp, gu8, gus, cnt, M, out=act)
    routed = [int(c) > 0 for c in cnt.tolist()]
    if kind == "edges":
        assert not routed[0] and not routed[-1] and any(routed)
    for e in range(E):
        got = act[e * slab:(e + 1) * slab]
        if routed[e]:
            want = torch.full((slab,), SENTINEL, dtype=torch.bfloat16, device=DEV)  # padding rows: not stored
            ops.linear_w8(xp, gu8[e], gus[e], M, out=want, epilogue=1, out_packed=True)
            assert torch.equal(got, want), f"expert {e}"
        else:
            assert bool((got == SENTINEL).all()), f"unrouted expert {e} was written"


@pytest.mark.parametrize("M", MS)
@pytest.mark.parametrize("H,F,E", SHAPES)
def test_down_with_one_expert_and_weight_one_equals_the_gemm_bit_for_bit(H, F, E, M, monkeypatch):
    assert ops.moe_w8_ok(M, E, H, F)
    monkeypatch.setattr(ops, "_W8_MODE", "rw")
    _, _, dn8, dns = expert_weights(H, F, E)
    act, _ = act_slabs(M, F, E, 10)
    slab = ops.packed_numel(M, F)
    for e in (E - 2, 0):
        wd, cnt = routing(M, E, ("one", e))
        y = ops.moe_down_w8(act, dn8, dns, cnt, wd, M)
        want = ops.linear_w8(act[e * slab:(e + 1) * slab], dn8[e], dns[e], M)
        assert torch.equal(y, want), f"expert {e}"


@pytest.mark.parametrize("kind", ["all", "edges"])
@pytest.mark.parametrize("M", MS)
@pytest.mark.parametrize("H,F,E", SHAPES)
def test_down_general_routing_matches_the_fp32_oracle(H, F, E, M, kind):
    """Error sources: fp32 summation order and one bf16 rounding - the bounds of
    test_w8a16_gemm_matches_dequantized_reference."""
    assert ops.moe_w8_ok(M, E, H, F)
    _, _, dn8, dns = expert_weights(H, F, E)
    act, xs = act_slabs(M, F, E, 20)
    wd, cnt = routing(M, E, kind)
    y = ops.moe_down_w8(act, dn8, dns, cnt, wd, M)
    want = down_oracle(xs, dn8, dns, wd)
    err = float((y.float() - want).norm() / want.norm())
    print(f"H={H} F={F} E={E} M={M} {kind}: max abs err {float((y.float() - want).abs().max()):.4g}, rel fro {err:.3g}")
    torch.testing.assert_close(y.float(), want, atol=5e-2, rtol=2e-2)
    assert err < 1e-2


@pytest.mark.parametrize("M", [13, 64])
@pytest.mark.parametrize("H,F,E", SHAPES)
def test_unrouted_experts_are_never_read(H, F, E, M):
    """e4m3 NaN codes over every unrouted expert's weights and NaN over its activation slab."""
    assert ops.moe_w8_ok(M, E, H, F)
    gu8, gus, dn8, dns = expert_weights(H, F, E)
    xp = ops.pack_act(rows(M, H, 1))
    wd, cnt = routing(M, E, "edges")
    slab = ops.packed_numel(M, F)
    act = ops.moe_gate_up_w8(xp, gu8, gus, cnt, M)
    act_in, _ = act_slabs(M, F, E, 20)
    y = ops.moe_down_w8(act_in, dn8, dns, cnt, wd, M)
    gu8n, dn8n, act_n = gu8.clone(), dn8.clone(), act_in.clone()
    for e, c in enumerate(cnt.tolist()):
        if c == 0:
            gu8n[e] = 0x7F
            dn8n[e] = 0x7F
            act_n[e * slab:(e + 1) * slab] = float("nan")
    act2 = ops.moe_gate_up_w8(xp, gu8n, gus, cnt, M)
    y2 = ops.moe_down_w8(act_n, dn8n, dns, cnt, wd, M)
    for e, c in enumerate(cnt.tolist()):
        if c > 0:
            assert torch.equal(act2[e * slab:(e + 1) * slab], act[e * slab:(e + 1) * slab])
    assert torch.isfinite(y2.float()).all() and torch.equal(y2, y)
    assert torch.isfinite(ops.unpack_act(act2[slab:2 * slab], M, F).float()).all()


@pytest.mark.parametrize("M", [13, 50])
@pytest.mark.parametrize("H,F,E", SHAPES)
def test_padding_rows_past_m_are_never_read_into_a_result_row(H, F, E, M):
    assert ops.moe_w8_ok(M, E, H, F)
    gu8, gus, dn8, dns = expert_weights(H, F, E)
    wd, cnt = routing(M, E, "all")
    slab = ops.packed_numel(M, F)
    x = rows(M, H, 1)
    act = ops.moe_gate_up_w8(pack_padded(x, 0.0), gu8, gus, cnt, M)
    act2 = ops.moe_gate_up_w8(pack_padded(x, float("nan")), gu8, gus, cnt, M)
    for e in range(E):
        a, b = (ops.unpack_act(t[e * slab:(e + 1) * slab], M, F) for t in (act, act2))
        assert torch.equal(a, b) and torch.isfinite(b.float()).all()
    a0, _ = act_slabs(M, F, E, 20, pad=0.0)
    a1, _ = act_slabs(M, F, E, 20, pad=float("nan"))
    assert not torch.isfinite(a1.float()).all()
    y = ops.moe_down_w8(a0, dn8, dns, cnt, wd, M)
    y2 = ops.moe_down_w8(a1, dn8, dns, cnt, wd, M)
    assert torch.isfinite(y2.float()).all() and torch.equal(y2, y)


def test_uncovered_shapes_and_bad_arguments_launch_nothing():
    assert not ops.moe_w8_ok(65, 4, 256, 256) and not ops.moe_w8_ok(4, 33, 256, 256)
    assert not ops.moe_w8_ok(4, 4, 256, 96) and not ops.moe_w8_ok(0, 4, 256, 256)
    gu8, gus, dn8, dns = expert_weights(256, 256, 4)
    xp = ops.pack_act(rows(4, 256, 1))
    wd, cnt = routing(4, 4, "all")
    with pytest.raises(RuntimeError, match="cnt"):
        torch.ops.mpamd.moe_gate_up_w8(xp, gu8, gus, cnt.long(), torch.empty(4 * 16 * 256, dtype=torch.bfloat16,
                                                                           device=DEV), 4)
    with pytest.raises(RuntimeError, match="act"):
        torch.ops.mpamd.moe_gate_up_w8(xp, gu8, gus, cnt, torch.empty(16, dtype=torch.bfloat16, device=DEV), 4)
    act = ops.moe_gate_up_w8(xp, gu8, gus, cnt, 4)
    with pytest.raises(RuntimeError, match="wd"):
        torch.ops.mpamd.moe_down_w8(act, dn8, dns, cnt, wd.double(), torch.empty(4, 256, dtype=torch.bfloat16,
                                                                                 device=DEV), 4)
    with pytest.raises(RuntimeError, match="y shape"):
        torch.ops.mpamd.moe_down_w8(act, dn8, dns, cnt, wd, torch.empty(4, 128, dtype=torch.bfloat16, device=DEV), 4)
    torch.cuda.synchronize()


# ------------------------------------------------------------------ executor
def _fp8_mixtral(seed=4):
    cfg = resolve_model("tiny-mixtral")
    mk = lambda **kw: random_stage_weights(cfg, 0, cfg.num_hidden_layers, has_embed=True, has_head=True,  # noqa: E731
                                           device=DEV, dtype=torch.bfloat16, seed=seed, **kw)
    return cfg, mk, dequantized(mk(), torch.float32)


def _count_grouped(monkeypatch):
    calls = {"gate_up": 0, "down": 0}
    gu, dn = ops.moe_gate_up_w8, ops.moe_down_w8

    def gate_up(*a, **kw):
        calls["gate_up"] += 1
        return gu(*a, **kw)

    def down(*a, **kw):
        calls["down"] += 1
        return dn(*a, **kw)

    monkeypatch.setattr(ops, "moe_gate_up_w8", gate_up)
    monkeypatch.setattr(ops, "moe_down_w8", down)
    return calls


def _generate(ex, cfg, oracle, steps=5):
    """Prompts and steps of test_mixtral_gpu_matches_fp32_reference, its bound against the fp32 oracle
    over the dequantized weights; returns every step's logits."""
    g = torch.Generator().manual_seed(0)
    prompts = [torch.randint(0, cfg.vocab_size, (n,), generator=g) for n in (80, 9)]
    logits = ex.forward([("a", 80), ("b", 9)], torch.cat(prompts).cuda())
    seqs = [p.clone() for p in prompts]
    out = []
    for _ in range(steps):
        out.append(logits.clone())
        for i, p in enumerate(seqs):
            r = reference_forward([oracle], p.cuda())[-1]
            torch.testing.assert_close(logits[i].float(), r, atol=0.06, rtol=0.05)
        nxt = torch.argmax(logits.float(), -1)
        seqs = [torch.cat([s, nxt[i:i + 1].cpu()]) for i, s in enumerate(seqs)]
        logits = ex.forward([("a", 1), ("b", 1)], nxt)
    return out


def test_fp8_mixtral_executor_matches_oracle_graphs_bit_equal_and_runs_the_grouped_ops(monkeypatch):
    cfg, mk, oracle = _fp8_mixtral()
    assert ops.moe_w8_ok(2, cfg.num_local_experts, cfg.hidden_size, cfg.intermediate_size)
    calls = _count_grouped(monkeypatch)
    runs = {}
    for graphs in (False, True):
        w = mk(quant_type="fp8")
        ex = StageExecutor(cfg, w, DEV, kv_cache_bytes=128 << 20, max_sessions=4, max_seq_len=256, use_graphs=graphs)
        L = w.layers[0]
        assert ex.quant_type == "fp8" and ex._moe_w8 and L.w8 and not L.folded and L.gate_up is None
        assert L.gate_up_w8.shape[0] == cfg.num_local_experts and L.router_p is not None
        assert ex.graph_max_batch <= 64
        before = dict(calls)
        runs[graphs] = _generate(ex, cfg, oracle)
        assert calls["gate_up"] > before["gate_up"] and calls["down"] > before["down"]
        if graphs:
            assert ex.last_graphed
    for a, b in zip(runs[False], runs[True]):
        assert torch.equal(a, b)


def test_fp8_mixtral_ungrouped_switch_runs_expert_by_expert(monkeypatch):
    cfg, mk, oracle = _fp8_mixtral()
    monkeypatch.setenv("MPAMD_MOE_GROUPED", "0")
    calls = _count_grouped(monkeypatch)
    ex = StageExecutor(cfg, mk(quant_type="fp8"), DEV, kv_cache_bytes=128 << 20, max_sessions=4, max_seq_len=256,
                       use_graphs=True)
    _generate(ex, cfg, oracle)
    assert calls == {"gate_up": 0, "down": 0}


def test_fp8_mixtral_65_session_decode_step_takes_the_dequantizing_path(monkeypatch):
    cfg, mk, oracle = _fp8_mixtral()
    calls = _count_grouped(monkeypatch)
    ex = StageExecutor(cfg, mk(quant_type="fp8"), DEV, kv_cache_bytes=128 << 20, max_sessions=80, max_seq_len=64,
                       use_graphs=True, warmup=False)
    n, plen = 65, 3
    g = torch.Generator().manual_seed(3)
    prompts = torch.randint(0, cfg.vocab_size, (n, plen), generator=g)
    seqs = [(f"s{i}", plen) for i in range(n)]
    logits = ex.forward(seqs, prompts.reshape(-1).cuda())
    nxt = torch.argmax(logits.float(), -1)
    logits = ex.forward([(f"s{i}", 1) for i in range(n)], nxt)
    assert not ex.last_graphed and calls == {"gate_up": 0, "down": 0}
    for i in (0, 64):
        ids = torch.cat([prompts[i], nxt[i:i + 1].cpu()]).cuda()
        torch.testing.assert_close(logits[i].float(), reference_forward([oracle], ids)[-1], atol=0.06, rtol=0.05)


@pytest.mark.parametrize("mode", ["w8a8", "mx"])
def test_other_fp8_modes_raise_for_moe(mode, monkeypatch):
    cfg, mk, _ = _fp8_mixtral()
    monkeypatch.setenv("MPAMD_FP8_MODE", mode)
    with pytest.raises(ValueError, match="MoE"):
        StageExecutor(cfg, mk(quant_type="fp8"), DEV, kv_cache_bytes=16 << 20, max_sessions=2, max_seq_len=64)
