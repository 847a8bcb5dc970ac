"""fp8 (e4m3, W8A16) weights for Mixtral - the CPU side: quantized expert stacks, the loaders, the
dequantizing executor path against the fp32 oracle over the dequantized weights, the torch forms of the
two grouped MoE ops (ops.moe_gate_up_w8 / moe_down_w8) against a direct fp32 formula, block sizes, a
stage server with ``--quant_type int8`` and the combinations that must raise.  The kernels themselves:
tests/test_moe_fp8_gpu.py.
"""
import types

import pytest
import torch

from src import ops
from src.block_utils import get_block_size
from src.llama_partition import load_stage_model
from src.models.config import resolve_model
from src.models.reference_model import greedy_generate, reference_forward
from src.models.weights import LlamaLayer, StageWeights, random_stage_weights
from src.ops import moe
from src.ops import reference as ref
from src.runtime.executor import StageExecutor


def _stage(cfg, dtype=torch.float32, seed=11, start=0, end=None, embed=True, head=True, **kw):
    end = cfg.num_hidden_layers if end is None else end
    return random_stage_weights(cfg, start, end, has_embed=embed, has_head=head, device="cpu", dtype=dtype, seed=seed,
                                **kw)


def dequantized(w: StageWeights, dtype=torch.float32) -> StageWeights:
    """Unquantized weights -> the same stage with every projection replaced by dequant(quant(W)),
    expert by expert: what an fp8 stage computes with, as plain row-major matrices for the oracle."""
    for L in w.layers:
        for name in LlamaLayer.PROJ:
            t = getattr(L, name)
            if t.dim() == 3:
                t = torch.stack([ops.unpack_weight_fp8(*ops.pack_weight_fp8(t[e]), dtype) for e in range(t.shape[0])])
            else:
                t = ops.unpack_weight_fp8(*ops.pack_weight_fp8(t), dtype)
            setattr(L, name, t)
    return w


def test_quantized_mixtral_weights_layout():
    cfg = resolve_model("tiny-mixtral")
    E, H, F = cfg.num_local_experts, cfg.hidden_size, cfg.intermediate_size
    for kw in (dict(quant_type="fp8"), dict(fp8=True)):
        w = _stage(cfg, torch.bfloat16, end=1, embed=False, head=False, **kw)
        L = w.layers[0]
        assert w.fp8 and L.fp8 and not L.w8
        assert L.gate_up is None and L.down is None and L.qkv is None and L.o is None
        assert L.gate_up_q.shape == (E, 2 * F // 16, H // 64, 64, 16) and L.gate_up_q.dtype == torch.uint8
        assert L.gate_up_s.shape == (E, 2 * F) and L.gate_up_s.dtype == torch.float32
        assert L.down_q.shape == (E, H // 16, F // 64, 64, 16) and L.down_s.shape == (E, H)
        assert L.qkv_q.dim() == 4 and L.o_q.dim() == 4
        assert L.router is not None and L.router.dtype == torch.bfloat16 and L.router.shape == (E, H)
        assert L.input_norm.dtype == torch.bfloat16 and not L.folded
    # W8A16 conversion: stacked per expert, no norm folding, no second quantization
    ref_w = dequantized(_stage(cfg, torch.bfloat16, end=1, embed=False, head=False))
    w.prepare_w8a16(fold_norms=True)
    L = w.layers[0]
    assert L.w8 and not L.folded and L.gate_up_q is None
    assert L.gate_up_w8.shape == (E, 2 * F // 16, H // 32, 64, 8) and L.gate_up_ws.shape == (E, 2 * F)
    assert L.down_w8.shape == (E, H // 16, F // 32, 64, 8) and L.down_ws.shape == (E, H)
    for name in LlamaLayer.PROJ:
        assert torch.equal(L.dense(name, torch.float32), getattr(ref_w.layers[0], name))
    assert torch.equal(L.dense("down", torch.float32, expert=2), ref_w.layers[0].down[2])


def test_loaders_accept_fp8_and_keep_rejecting_4bit_for_moe():
    full = load_stage_model("tiny-mixtral", "cpu", "full", quant_type="int8")
    assert full.weights.fp8 and full.weights.layers[0].gate_up is None
    assert load_stage_model("tiny-mixtral", "cpu", "full", quant_type="fp8").weights.fp8
    for q in ("mxfp4", "nf4"):
        with pytest.raises(ValueError, match="MoE"):
            load_stage_model("tiny-mixtral", "cpu", "full", quant_type=q)


def test_cpu_executor_over_fp8_experts_matches_oracle_on_dequantized_weights():
    """Same arithmetic as test_sparse_and_dense_schedules_match_oracle (fp32, same weights): its bound."""
    cfg = resolve_model("tiny-mixtral")
    w = _stage(cfg, quant_type="fp8")
    wd = dequantized(_stage(cfg))
    ex = StageExecutor(cfg, w, "cpu", dtype=torch.float32, kv_cache_bytes=16 << 20, max_sessions=4, max_seq_len=256)
    assert ex.quant_type == "fp8" and not w.layers[0].folded and w.layers[0].gate_up is None
    g = torch.Generator().manual_seed(1)
    a = torch.randint(0, cfg.vocab_size, (90,), generator=g)   # > 64 rows: expert-grouped schedule
    b = torch.randint(0, cfg.vocab_size, (7,), generator=g)
    lg = ex.forward([("a", 90), ("b", 7)], torch.cat([a, b]))
    torch.testing.assert_close(lg[0], reference_forward([wd], a)[-1], atol=1e-4, rtol=1e-4)
    torch.testing.assert_close(lg[1], reference_forward([wd], b)[-1], atol=1e-4, rtol=1e-4)
    for _ in range(3):  # decode steps: the dense schedule
        nxt = torch.argmax(lg, -1)
        a, b = torch.cat([a, nxt[:1]]), torch.cat([b, nxt[1:]])
        lg = ex.forward([("a", 1), ("b", 1)], nxt)
        torch.testing.assert_close(lg[0], reference_forward([wd], a)[-1], atol=1e-4, rtol=1e-4)
        torch.testing.assert_close(lg[1], reference_forward([wd], b)[-1], atol=1e-4, rtol=1e-4)


# ------------------------------------------------------------------ torch forms of the grouped ops
def moe_case(M, H, F, E, routing, device="cpu", seed=0):
    """Inputs of the two grouped ops at test_w8a16_gemm_matches_dequantized_reference's scales
    (x ~ N(0, 1) in bf16, w ~ 0.02 N(0, 1)).  ``routing``: "all" (top-2, every expert routed when
    2 M >= E), "edges" (top-2 among the experts 1 .. E-2: first and last unrouted) or "top1"
    (expert 1 only, weight 1)."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(M, H, generator=g).to(torch.bfloat16)
    gu = 0.02 * torch.randn(E, 2 * F, H, generator=g)
    dn = 0.02 * torch.randn(E, H, F, generator=g)

    def stack(w):
        qs = [ops.pack_weight_fp8(w[e]) for e in range(E)]
        return torch.stack([ops.w8_from_fp8(q) for q, _ in qs]), torch.stack([s for _, s in qs])

    gu8, gus = stack(gu)
    dn8, dns = stack(dn)
    if routing == "top1":
        wd = torch.zeros(M, E)
        wd[:, 1] = 1.0
    else:
        logits = torch.randn(M, E, generator=g)
        if routing == "edges":
            logits[:, 0] = logits[:, E - 1] = -1e9
        wd = moe.dense_weights(*moe.route(logits, 2), E)
        if routing == "all" and 2 * M >= E:  # make sure every expert has a row
            for e in range(E):
                if not (wd[:, e] > 0).any():
                    r = e % M
                    wd[r] = 0
                    wd[r, e] = wd[r, (e + 1) % E] = 0.5
    cnt = (wd > 0).sum(0, dtype=torch.int32)
    to = lambda t: t.to(device)  # noqa: E731
    return dict(x=to(x), xp=ops.pack_act(to(x)), gu8=to(gu8), gus=to(gus), dn8=to(dn8), dns=to(dns), wd=to(wd),
                cnt=to(cnt), M=M, H=H, F=F, E=E)


def swiglu_oracle(c, e):
    """fp32 SwiGLU of expert e over the dequantized weight, rounded to bf16 where the kernel rounds."""
    y = (c["x"].float() @ ops.unpack_weight_w8(c["gu8"][e], c["gus"][e], torch.float32).t()).to(torch.bfloat16)
    return ref.swiglu(y)


def down_oracle(c, acts):
    """sum_e wd[:, e] * (act_e.float() @ dequant(down_e).T) in fp32 (``acts``: routed expert -> [M, F])."""
    tot = torch.zeros(c["M"], c["H"], dtype=torch.float32, device=c["x"].device)
    for e, a in acts.items():
        tot += c["wd"][:, e:e + 1] * (a.float() @ ops.unpack_weight_w8(c["dn8"][e], c["dns"][e], torch.float32).t())
    return tot


@pytest.mark.parametrize("routing", ["all", "edges", "top1"])
def test_torch_forms_of_the_grouped_ops_match_the_fp32_formula(routing):
    c = moe_case(13, 256, 256, 4, routing)
    M, F, E = c["M"], c["F"], c["E"]
    routed = [e for e in range(E) if int(c["cnt"][e]) > 0]
    assert routed == {"all": [0, 1, 2, 3], "edges": [1, 2], "top1": [1]}[routing]
    slab = ops.packed_numel(M, F)
    act = torch.full((E * slab,), 7.0, dtype=torch.bfloat16)
    out = ops.moe_gate_up_w8(c["xp"], c["gu8"], c["gus"], c["cnt"], M, out=act)
    assert out is act
    acts = {}
    for e in range(E):
        got = ops.unpack_act(act[e * slab:(e + 1) * slab], M, F)
        if e in routed:
            torch.testing.assert_close(got.float(), swiglu_oracle(c, e).float(), atol=1e-6, rtol=2 ** -7)
            acts[e] = got
        else:
            assert bool((act[e * slab:(e + 1) * slab] == 7.0).all())  # unrouted: slab untouched
    y = ops.moe_down_w8(act, c["dn8"], c["dns"], c["cnt"], c["wd"], M)
    want = down_oracle(c, acts)
    assert y.dtype == torch.bfloat16 and y.shape == (M, c["H"])
    # one bf16 rounding of the fp32 sum (2^-9 relative), fp32 summation-order noise beside it
    torch.testing.assert_close(y.float(), want, atol=1e-5, rtol=2 ** -8)
    if routing == "top1":  # weight 1: exactly the single expert's GEMM, rounded once
        assert torch.equal(y, want.to(torch.bfloat16))


def test_torch_forms_never_read_unrouted_experts():
    c = moe_case(13, 256, 256, 4, "edges")
    M, F, E = c["M"], c["F"], c["E"]
    slab = ops.packed_numel(M, F)
    act = ops.moe_gate_up_w8(c["xp"], c["gu8"], c["gus"], c["cnt"], M)
    y = ops.moe_down_w8(act, c["dn8"], c["dns"], c["cnt"], c["wd"], M)
    gu8, dn8, act2 = c["gu8"].clone(), c["dn8"].clone(), act.clone()
    for e in (0, E - 1):
        gu8[e] = 0x7F  # e4m3 NaN
        dn8[e] = 0x7F
        act2[e * slab:(e + 1) * slab] = float("nan")
    act3 = ops.moe_gate_up_w8(c["xp"], gu8, c["gus"], c["cnt"], M, out=act2.clone())
    for e in (1, 2):
        assert torch.equal(act3[e * slab:(e + 1) * slab], act[e * slab:(e + 1) * slab])
    y2 = ops.moe_down_w8(act2, dn8, c["dns"], c["cnt"], c["wd"], M)
    assert torch.isfinite(y2.float()).all() and torch.equal(y2, y)


def test_grouped_ops_check_their_arguments():
    c = moe_case(4, 256, 256, 4, "all")
    with pytest.raises(ValueError, match="w_scale"):
        ops.moe_gate_up_w8(c["xp"], c["gu8"], c["gus"][:, :-1], c["cnt"], 4)
    with pytest.raises(ValueError, match="cnt"):
        ops.moe_gate_up_w8(c["xp"], c["gu8"], c["gus"], c["cnt"].long(), 4)
    with pytest.raises(ValueError, match="rows"):
        ops.moe_gate_up_w8(c["xp"], c["gu8"], c["gus"], c["cnt"], 65)
    act = ops.moe_gate_up_w8(c["xp"], c["gu8"], c["gus"], c["cnt"], 4)
    with pytest.raises(ValueError, match="wd"):
        ops.moe_down_w8(act, c["dn8"], c["dns"], c["cnt"], c["wd"][:, :-1], 4)
    with pytest.raises(ValueError, match="w8"):
        ops.moe_down_w8(act, c["dn8"][0], c["dns"], c["cnt"], c["wd"], 4)


# ------------------------------------------------------------------ block sizes
def _formula(cfg, elt=2):
    H, F, E = cfg.hidden_size, cfg.intermediate_size, cfg.num_local_experts
    qkv_n = cfg.q_dim + 2 * cfg.kv_dim
    matrices = qkv_n * H + H * cfg.q_dim + E * 3 * H * F
    scales = qkv_n + H + E * (2 * F + H)
    return matrices + E * H * elt + 4 * scales + 2 * H * elt


@pytest.mark.parametrize("model", ["tiny-mixtral", "mixtral-8x7b"])
def test_block_size_of_an_fp8_mixtral_block(model):
    cfg = resolve_model(model)
    size = get_block_size(cfg, "memory", torch.bfloat16, "fp8")
    assert size == _formula(cfg) == get_block_size(cfg, "memory", torch.bfloat16, "int8")
    assert size < 0.52 * get_block_size(cfg, "memory", torch.bfloat16)
    if model == "tiny-mixtral":
        one = _stage(cfg, torch.bfloat16, start=1, end=2, embed=False, head=False, quant_type="fp8")
        assert one.nbytes() == size
    for q in ("mxfp4", "nf4"):
        with pytest.raises(ValueError, match="MoE"):
            get_block_size(cfg, "memory", torch.bfloat16, q)


# ------------------------------------------------------------------ serving
@pytest.mark.timeout(120)
def test_mixtral_stage_server_with_int8_generates_and_announces_fp8():
    """``--quant_type int8`` on a Mixtral stage server (CPU): the client's tokens equal greedy decoding over
    the unquantized first stage + the dequantized fp8 blocks; ``rpc_info`` and the announcement say fp8."""
    from src import main as M
    from src.comm.wire import Message
    from src.dht_utils import get_stage_key
    from src.models.tokenizer import load_tokenizer

    from .swarm_utils import ServerThread, client_args, server_argv

    model, cut = "tiny-mixtral", 2
    cfg = resolve_model(model)
    s1 = ServerThread(server_argv(model, str(cut), 1, extra="--quant_type int8")).wait()
    try:
        assert s1.srv.ex.quant_type == "fp8" and s1.srv.ex.w.fp8 and s1.srv.ex.w.layers[0].gate_up is None
        info = s1.srv.loop.run(s1.srv.handler.rpc_info(Message({}, [])), timeout=10)
        assert info.metadata["quant_type"] == "fp8"
        rec = s1.dht.get(get_stage_key(1), latest=True)
        assert "fp8" in repr(rec.value)
        args = client_args(model, str(cut), s1.addr, "--max_new_tokens 6 --temperature 0")
        gen = M.run_rank0(args, torch.device("cpu"), [cut])
        wdt = s1.srv.ex.dtype
    finally:
        s1.close()
    wd = random_stage_weights(cfg, 0, cfg.num_hidden_layers, has_embed=True, has_head=True, device="cpu", dtype=wdt,
                              seed=0)
    for L in wd.layers[cut:]:
        dequantized(StageWeights(cfg, 0, 1, [L]), wdt)
    ids = torch.tensor(load_tokenizer(model, cfg).encode("Hello, how are you?"))
    assert gen == greedy_generate([wd], ids, len(gen)) and len(gen) == 6


# ------------------------------------------------------------------ what must raise
def test_tensor_parallel_with_fp8_experts_raises():
    cfg = resolve_model("tiny-mixtral")
    w = _stage(cfg, quant_type="fp8")
    tp = types.SimpleNamespace(size=2, active=True, capturable=False)
    with pytest.raises(ValueError, match="MoE"):
        StageExecutor(cfg, w, "cpu", dtype=torch.float32, kv_cache_bytes=8 << 20, max_sessions=2, max_seq_len=64, tp=tp)
