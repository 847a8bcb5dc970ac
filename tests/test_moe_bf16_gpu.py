"""The grouped bf16 MoE kernels (csrc/gemm_moe_bf16.hip) and the MPAMD_MOE_GROUPED_BF16=1 executor route on the GPU.

Shapes and rows: the set of tests/test_moe_fp8_gpu.py (ring tail, every tile width, partial and full row tiles,
256 workgroups), none refused by ops.moe_ok.  Bounds: fp32 summation order plus one bf16 rounding; gate/up holds
it although its SwiGLU rounds the two products to bf16 first, as every SwiGLU epilogue here.
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

pytestmark = pytest.mark.gpu
DEV = "cuda"
SHAPES = [(256, 256, 4), (1152, 1152, 4), (256, 6144, 4), (6144, 256, 4), (256, 14336, 8), (4096, 256, 8)]
MS = [1, 13, 16, 17, 50, 64]
SENTINEL = 7.0
NAN = float("nan")


@functools.lru_cache(maxsize=None)
def expert_weights(H, F, E):
    """(gate_up [E, 2F, H], down [E, H, F]) bf16 ~ 0.02 N(0, 1) and their packed stacks."""
    g = torch.Generator(device=DEV).manual_seed(H * 31 + F * 7 + E)
    gu = (0.02 * torch.randn(E, 2 * F, H, device=DEV, generator=g)).to(torch.bfloat16)
    dn = (0.02 * torch.randn(E, H, F, device=DEV, generator=g)).to(torch.bfloat16)
    return gu, dn, torch.stack([ops.pack_weight(w) for w in gu]), torch.stack([ops.pack_weight(w) for w in dn])


def routing(M, E, kind):
    """wd fp32 [M, E] + counts: top-2 over "all" experts or with the "edges" unrouted; int e: e alone, weight 1."""
    if isinstance(kind, int):
        wd = torch.zeros(M, E, device=DEV)
        wd[:, kind] = 1.0
    else:
        logits = torch.randn(M, E, device=DEV, generator=torch.Generator(device=DEV).manual_seed(M))
        if kind == "edges":
            logits[:, 0] = logits[:, E - 1] = -1e9
        wd = moe.dense_weights(*moe.route(logits, 2), E)
    return wd, (wd > 0).sum(0, dtype=torch.int32)


def rows(M, K, seed):
    return torch.randn(M, K, device=DEV, generator=torch.Generator(device=DEV).manual_seed(seed)).to(torch.bfloat16)


def pack_padded(x, pad):
    full = torch.full((((x.shape[0] + 15) // 16) * 16, x.shape[1]), pad, dtype=x.dtype, device=x.device)
    full[:x.shape[0]] = x
    return ops.pack_act(full)


def act_slabs(M, F, E, pad=0.0):
    xs = [rows(M, F, 20 + e) for e in range(E)]
    return torch.cat([pack_padded(x, pad) for x in xs]), xs


def close(got, want, what):
    err = float((got.float() - want).norm() / want.norm())
    print(f"{what}: max abs err {float((got.float() - want).abs().max()):.4g}, rel fro {err:.3g}")
    torch.testing.assert_close(got.float(), want, atol=5e-2, rtol=2e-2)
    assert err < 1e-2


@pytest.mark.parametrize("kind", ["all", "edges"])
@pytest.mark.parametrize("M", MS)
@pytest.mark.parametrize("H,F,E", SHAPES)
def test_gate_up_and_down_match_the_fp32_formula(H, F, E, M, kind):
    assert ops.moe_ok(M, E, H, F)
    gu, dn, gup, dnp = expert_weights(H, F, E)
    x = rows(M, H, 1)
    wd, cnt = routing(M, E, kind)
    assert kind == "all" or (int(cnt[0]) == int(cnt[-1]) == 0 and int(cnt.sum()) == 2 * M)
    slab = ops.packed_numel(M, F)
    act = torch.full((E * slab,), SENTINEL, dtype=torch.bfloat16, device=DEV)
    ops.moe_gate_up(ops.pack_act(x), gup, cnt, M, out=act)
    act_in, xs = act_slabs(M, F, E)
    y = ops.moe_down(act_in, dnp, cnt, wd, M)
    want = torch.zeros(M, H, device=DEV)
    for e, c in enumerate(cnt.tolist()):
        if c == 0:
            assert bool((act[e * slab:(e + 1) * slab] == SENTINEL).all()), f"unrouted expert {e} was written"
            continue
        p = (x.float() @ gu[e].float().t()).view(M, F // 16, 2, 16)
        swi = (torch.nn.functional.silu(p[:, :, 0]) * p[:, :, 1]).reshape(M, F).to(torch.bfloat16)
        close(ops.unpack_act(act[e * slab:(e + 1) * slab], M, F), swi.float(), f"gate/up e{e}")
        want += wd[:, e:e + 1] * (xs[e].float() @ dn[e].float().t())
    close(y, want, "down")
    assert torch.equal(ops.moe_down(act_in, dnp, cnt, wd, M), y)  # the same bits on every run
    assert torch.equal(ops.moe_gate_up(ops.pack_act(x), gup, cnt, M, out=torch.full_like(act, SENTINEL)), act)


@pytest.mark.parametrize("M", MS)
@pytest.mark.parametrize("H,F,E", SHAPES)
def test_one_expert_with_weight_one_equals_the_ring_gemm_bit_for_bit(H, F, E, M, monkeypatch):
    monkeypatch.setattr(ops, "_GEMM_SK", "rw")  # ops.linear on its ring form
    _, _, gup, dnp = expert_weights(H, F, E)
    xp = ops.pack_act(rows(M, H, 1))
    act_in, _ = act_slabs(M, F, E)
    slab = ops.packed_numel(M, F)
    for e in (E - 2, 0):
        wd, cnt = routing(M, E, e)
        act = ops.moe_gate_up(xp, gup, cnt, M)
        want = torch.zeros(slab, dtype=torch.bfloat16, device=DEV)
        ops.linear(xp, None, out=want, epilogue=1, wp=gup[e], a_rows=M, out_packed=True)
        assert torch.equal(act[e * slab:(e + 1) * slab], want), f"gate/up expert {e}"
        y = ops.moe_down(act_in, dnp, cnt, wd, M)
        assert torch.equal(y, ops.linear(act_in[e * slab:(e + 1) * slab], None, wp=dnp[e], a_rows=M)), f"down {e}"


@pytest.mark.parametrize("M,pad", [(13, 0.0), (64, 0.0), (13, NAN), (50, NAN)])
@pytest.mark.parametrize("H,F,E", SHAPES)
def test_unrouted_experts_and_padding_rows_are_never_read(H, F, E, M, pad):
    """NaN over every unrouted expert's weights and slab, and (M 13, 50) in the packed padding rows."""
    _, _, gup, dnp = expert_weights(H, F, E)
    x = rows(M, H, 1)
    wd, cnt = routing(M, E, "edges")
    slab = ops.packed_numel(M, F)
    act = ops.moe_gate_up(pack_padded(x, 0.0), gup, cnt, M)
    act_in, _ = act_slabs(M, F, E)
    y = ops.moe_down(act_in, dnp, cnt, wd, M)
    gun, dnn = gup.clone(), dnp.clone()
    act_n, _ = act_slabs(M, F, E, pad=pad)
    for e, c in enumerate(cnt.tolist()):
        if c == 0:
            gun[e] = dnn[e] = NAN
            act_n[e * slab:(e + 1) * slab] = NAN
    assert not torch.isfinite(act_n.float()).all()
    act2 = ops.moe_gate_up(pack_padded(x, pad), gun, cnt, M)
    for e, c in enumerate(cnt.tolist()):
        if c > 0:
            a, b = (ops.unpack_act(t[e * slab:(e + 1) * slab], M, F) for t in (act, act2))
            assert torch.equal(a, b) and torch.isfinite(b.float()).all()
    y2 = ops.moe_down(act_n, dnn, cnt, wd, M)
    assert torch.isfinite(y2.float()).all() and torch.equal(y2, y)


def test_uncovered_shapes_and_bad_arguments_launch_nothing():
    assert not ops.moe_ok(65, 4, 256, 256) and not ops.moe_ok(4, 33, 256, 256)
    assert not ops.moe_ok(4, 4, 256, 96) and not ops.moe_ok(0, 4, 256, 256)
    _, _, gup, dnp = expert_weights(256, 256, 4)
    xp = ops.pack_act(rows(4, 256, 1))
    wd, cnt = routing(4, 4, "all")
    out = lambda *s: torch.empty(*s, dtype=torch.bfloat16, device=DEV)  # noqa: E731
    with pytest.raises(RuntimeError, match="cnt"):
        torch.ops.mpamd.moe_gate_up(xp, gup, cnt.long(), out(4 * 16 * 256), 4)
    with pytest.raises(RuntimeError, match="y shape"):
        torch.ops.mpamd.moe_down(out(4 * 16 * 256), dnp, cnt, wd, out(4, 128), 4)
    with pytest.raises(RuntimeError, match="no grouped kernel"):  # F = 96
        torch.ops.mpamd.moe_down(out(4 * 16 * 96), out(4, 16, 3, 64, 8), cnt, wd, out(4, 256), 4)
    torch.cuda.synchronize()


@pytest.mark.parametrize("switch", [True, False])
def test_bf16_mixtral_executor_on_the_grouped_route(switch, monkeypatch):
    """Steps and bound of test_mixtral_gpu_matches_fp32_reference; graphed steps equal the eager ones bit for bit."""
    cfg = resolve_model("tiny-mixtral")
    calls = []
    for name in ("moe_gate_up", "moe_down"):
        fn = getattr(ops, name)
        monkeypatch.setattr(ops, name, lambda *a, _f=fn, _n=name, **kw: (calls.append(_n), _f(*a, **kw))[1])
    if switch:
        monkeypatch.setenv("MPAMD_MOE_GROUPED_BF16", "1")
    else:
        monkeypatch.delenv("MPAMD_MOE_GROUPED_BF16", raising=False)
    runs = {}
    for graphs in (False, True):
        w = random_stage_weights(cfg, 0, cfg.num_hidden_layers, has_embed=True, has_head=True, device=DEV,
                                 dtype=torch.bfloat16, seed=4)
        ex = StageExecutor(cfg, w, DEV, kv_cache_bytes=128 << 20, max_sessions=4, max_seq_len=256, use_graphs=graphs)
        g = torch.Generator().manual_seed(0)
        seqs = [torch.randint(0, cfg.vocab_size, (n,), generator=g) for n in (80, 9)]
        logits = ex.forward([("a", 80), ("b", 9)], torch.cat(seqs).cuda())
        runs[graphs] = []
        for _ in range(5):
            runs[graphs].append(logits.clone())
            for i, p in enumerate(seqs):
                r = reference_forward([w], p.cuda())[-1]
                torch.testing.assert_close(logits[i].float(), r, atol=0.06, rtol=0.05)
            nxt = torch.argmax(logits.float(), -1)
            seqs = [torch.cat([s, nxt[i:i + 1].cpu()]) for i, s in enumerate(seqs)]
            logits = ex.forward([("a", 1), ("b", 1)], nxt)
        assert ex.last_graphed or not graphs
    assert all(torch.equal(a, b) for a, b in zip(runs[False], runs[True]))
    assert ("moe_gate_up" in calls and "moe_down" in calls) if switch else not calls
