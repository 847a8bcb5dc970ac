"""Grouped MoE ops over unquantized expert stacks (ops.moe_gate_up / moe_down) - the CPU side: their torch
forms against the fp32 formula, unrouted experts never read, the argument checks, and a CPU tiny-mixtral
executor on the MPAMD_MOE_GROUPED_BF16=1 route.  The kernels themselves: tests/test_moe_bf16_gpu.py.
"""
import pytest
import torch

from src import ops
from src.models.config import resolve_model
from src.models.reference_model import reference_forward
from src.models.weights import random_stage_weights
from src.ops import moe
from src.ops import reference as ref
from src.runtime.executor import StageExecutor


def moe_case(M, H, F, E, routing, seed=0):
    """Inputs and "all" / "edges" (first and last expert unrouted) top-2 routing of test_moe_fp8.py::moe_case."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(M, H, generator=g).to(torch.bfloat16)
    gu = (0.02 * torch.randn(E, 2 * F, H, generator=g)).to(torch.bfloat16)
    dn = (0.02 * torch.randn(E, H, F, generator=g)).to(torch.bfloat16)
    logits = torch.randn(M, E, generator=g)
    if routing == "edges":
        logits[:, 0] = logits[:, E - 1] = -1e9
    wd = moe.dense_weights(*moe.route(logits, 2), E)
    cnt = (wd > 0).sum(0, dtype=torch.int32)
    return dict(x=x, xp=ops.pack_act(x), gu=gu, dn=dn, gup=torch.stack([ops.pack_weight(w) for w in gu]),
                dnp=torch.stack([ops.pack_weight(w) for w in dn]), wd=wd, cnt=cnt)


@pytest.mark.parametrize("routing", ["all", "edges"])
def test_torch_forms_match_the_fp32_formula_and_never_read_unrouted_experts(routing):
    M, H, F, E = 13, 256, 256, 4
    c = moe_case(M, H, F, E, routing)
    routed = [e for e in range(E) if int(c["cnt"][e]) > 0]
    assert routed == {"all": [0, 1, 2, 3], "edges": [1, 2]}[routing]
    slab = ops.packed_numel(M, F)
    act = torch.full((E * slab,), 7.0, dtype=torch.bfloat16)
    for e in set(range(E)) - set(routed):  # NaN over everything of an unrouted expert
        c["gup"][e] = c["dnp"][e] = float("nan")
    assert ops.moe_gate_up(c["xp"], c["gup"], c["cnt"], M, out=act) is act
    want = torch.zeros(M, H)
    for e in range(E):
        if e not in routed:
            assert bool((act[e * slab:(e + 1) * slab] == 7.0).all())  # unrouted: slab untouched
            act[e * slab:(e + 1) * slab] = float("nan")
            continue
        got = ops.unpack_act(act[e * slab:(e + 1) * slab], M, F)
        y = (c["x"].float() @ c["gu"][e].float().t()).to(torch.bfloat16)
        torch.testing.assert_close(got.float(), ref.swiglu(y).float(), atol=1e-6, rtol=2 ** -7)
        want += c["wd"][:, e:e + 1] * (got.float() @ c["dn"][e].float().t())
    y = ops.moe_down(act, c["dnp"], c["cnt"], c["wd"], M)
    assert y.dtype == torch.bfloat16 and y.shape == (M, H) and torch.isfinite(y.float()).all()
    torch.testing.assert_close(y.float(), want, atol=1e-5, rtol=2 ** -8)  # one bf16 rounding of the fp32 sum


def test_grouped_ops_check_their_arguments():
    c = moe_case(4, 256, 256, 4, "all")
    with pytest.raises(ValueError, match="wp"):
        ops.moe_gate_up(c["xp"], c["gup"][0], c["cnt"], 4)
    with pytest.raises(ValueError, match="cnt"):
        ops.moe_gate_up(c["xp"], c["gup"], c["cnt"].long(), 4)
    with pytest.raises(ValueError, match="rows"):
        ops.moe_gate_up(c["xp"], c["gup"], c["cnt"], 65)
    act = ops.moe_gate_up(c["xp"], c["gup"], c["cnt"], 4)
    with pytest.raises(ValueError, match="wd"):
        ops.moe_down(act, c["dnp"], c["cnt"], c["wd"][:, :-1], 4)
    with pytest.raises(ValueError, match="wp"):
        ops.moe_down(act, c["dnp"][0], c["cnt"], c["wd"], 4)


@pytest.mark.parametrize("switch", [True, False])
def test_cpu_executor_takes_the_grouped_route_only_with_the_switch(switch, monkeypatch):
    """The bound of test_sparse_and_dense_schedules_match_oracle (fp32 arithmetic over the same weights)."""
    calls = []
    for name in ("moe_gate_up", "moe_down"):
        fn = getattr(ops, name)
        monkeypatch.setattr(ops, name, lambda *a, _f=fn, _n=name, **kw: (calls.append(_n), _f(*a, **kw))[1])
    if switch:
        monkeypatch.setenv("MPAMD_MOE_GROUPED_BF16", "1")
    else:
        monkeypatch.delenv("MPAMD_MOE_GROUPED_BF16", raising=False)
    cfg = resolve_model("tiny-mixtral")
    w = random_stage_weights(cfg, 0, cfg.num_hidden_layers, has_embed=True, has_head=True, device="cpu",
                             dtype=torch.float32, seed=11)
    ex = StageExecutor(cfg, w, "cpu", dtype=torch.float32, kv_cache_bytes=16 << 20, max_sessions=4, max_seq_len=256)
    g = torch.Generator().manual_seed(1)
    a, b = (torch.randint(0, cfg.vocab_size, (n,), generator=g) for n in (90, 7))  # 97 rows: never the grouped route
    lg = ex.forward([("a", 90), ("b", 7)], torch.cat([a, b]))
    assert not calls
    for _ in range(3):
        nxt = torch.argmax(lg, -1)
        a, b = torch.cat([a, nxt[:1]]), torch.cat([b, nxt[1:]])
        lg = ex.forward([("a", 1), ("b", 1)], nxt)
        torch.testing.assert_close(lg[0], reference_forward([w], a)[-1], atol=1e-4, rtol=1e-4)
        torch.testing.assert_close(lg[1], reference_forward([w], b)[-1], atol=1e-4, rtol=1e-4)
    n = 3 * cfg.num_hidden_layers
    assert calls.count("moe_gate_up") == calls.count("moe_down") == (n if switch else 0)
