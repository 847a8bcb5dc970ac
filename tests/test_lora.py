"""LoRA adapters on the CPU data path: the PEFT loader, the torch forms of the LoRA ops, the executor's
per-session adapters against a dense oracle on merged weights, the serving surface and a small swarm.

Bounds of the torch forms (derived; bf16 x bf16 products are exact in fp32):
  shrink:  |t - t64| <= 2 K 2^-24 scale sum_k |A x|_k
  expand, given the fp32 t: |y' - y64| <= 2^-8 |y64| + 2 (R + 2) 2^-24 (|y| + sum_j |B t|_j)
"""
import asyncio
import json
import math
import os
import types

import numpy as np
import pytest
import torch

from src import main as M
from src import ops
from src.block_utils import adapter_bytes_per_block, auto_num_blocks, get_block_size, kv_cache_bytes_per_block
from src.comm.wire import Message
from src.dht_utils import get_stage_key
from src.llama_partition import load_stage_model
from src.models import adapters as ad
from src.models.config import resolve_model
from src.models.reference_model import greedy_generate, reference_forward
from src.models.tokenizer import load_tokenizer
from src.models.weights import interleave_gate_up, random_stage_weights, split_gate_up
from src.rpc_handler import StageConnectionHandler
from src.runtime.executor import StageExecutor

from .swarm_utils import ServerThread, client_args, server_argv, wait_for

MODEL = "tiny-llama"
SEED = 7


def write_peft(path, cfg, rank, alpha, modules, layers=None, seed=0, bad_layers=(), **config):
    """A PEFT LoRA directory.  Entries are small multiples of 2^-6, so every product and every sum of
    ``B A`` is exact in fp32 whatever the summation order: 'equal in fp32' can be asked bit for bit.
    ``bad_layers`` get matrices of a shape no model fits (a loader that reads them raises)."""
    from safetensors.torch import save_file

    os.makedirs(path, exist_ok=True)
    g = torch.Generator().manual_seed(seed)
    tensors = {}
    for i in (range(cfg.num_hidden_layers) if layers is None else layers):
        for mod in modules:
            N, K = ad.module_shape(cfg, mod)
            shape_a, shape_b = ((1, 3), (3, 1)) if i in bad_layers else ((rank, K), (N, rank))
            tensors[ad.hf_key(i, mod, "A")] = torch.randint(-3, 4, shape_a, generator=g).float() / 64
            tensors[ad.hf_key(i, mod, "B")] = torch.randint(-3, 4, shape_b, generator=g).float() / 64
    save_file(tensors, os.path.join(path, ad.WEIGHT_FILE))
    c = {"peft_type": "LORA", "r": rank, "lora_alpha": alpha, "target_modules": list(modules), "bias": "none",
         "lora_dropout": 0.1, "use_rslora": False}
    c.update(config)
    with open(os.path.join(path, ad.CONFIG_FILE), "w") as f:
        json.dump(c, f)
    return tensors


def stage_weights(start=0, end=None, embed=True, head=True, dtype=torch.float32, model=MODEL, **kw):
    cfg = resolve_model(model)
    end = cfg.num_hidden_layers if end is None else end
    return cfg, random_stage_weights(cfg, start, end, has_embed=embed, has_head=head, device="cpu", dtype=dtype,
                                     seed=SEED, **kw)


@pytest.fixture(scope="module")
def peft_dirs(tmp_path_factory):
    """Adapter ``a``: all seven modules, r = 8, alpha = 16; adapter ``b``: q and v, r = 8, rslora."""
    cfg = resolve_model(MODEL)
    root = tmp_path_factory.mktemp("adapters")
    a, b = str(root / "a"), str(root / "b")
    ta = write_peft(a, cfg, 8, 16, ad.MODULES, seed=1)
    tb = write_peft(b, cfg, 8, 16, ("q_proj", "v_proj"), seed=2, use_rslora=True)
    return {"a": a, "b": b, "ta": ta, "tb": tb}


# ------------------------------------------------------------------------------------------- loader
def test_stacks_equal_the_fused_merged_hf_matrices_exactly(tmp_path):
    cfg, w = stage_weights(1, 3, embed=False, head=False)
    d = str(tmp_path / "mine")
    t = write_peft(d, cfg, 8, 16, ad.MODULES, seed=3, bad_layers=(0, 3))  # only layers 1 and 2 may be read
    lora = w.load_adapters([d])
    assert lora.names == ["mine"] and lora.scale.tolist() == [2.0]
    assert lora.ranks == {"qkv": 32, "o": 16, "gate_up": 16, "down": 16}
    scale = 2.0
    for li, i in enumerate((1, 2)):
        lay, L = w.layers[li], lora.layers[li]
        q, k, v = lay.qkv.split([cfg.q_dim, cfg.kv_dim, cfg.kv_dim])
        gate, up = split_gate_up(lay.gate_up)
        base = {"q_proj": q, "k_proj": k, "v_proj": v, "o_proj": lay.o, "gate_proj": gate, "up_proj": up,
                "down_proj": lay.down}
        m = {mod: base[mod].float() + scale * (t[ad.hf_key(i, mod, "B")] @ t[ad.hf_key(i, mod, "A")])
             for mod in ad.MODULES}
        want = {"qkv": torch.cat([m["q_proj"], m["k_proj"], m["v_proj"]]), "o": m["o_proj"],
                "gate_up": interleave_gate_up(m["gate_proj"], m["up_proj"]), "down": m["down_proj"]}
        for p in ad.FUSED:
            lp = getattr(L, p)
            assert lp.A.shape == (1, lora.ranks[p], getattr(lay, p).shape[1]) and lp.A.dtype == torch.float32
            got = getattr(lay, p).float() + lora.scale[0] * (lp.B[0].float() @ lp.A[0].float())
            assert torch.equal(got, want[p]), (i, p)
    # an untargeted projection has no storage, an untargeted module no rank columns
    cfg, w2 = stage_weights(1, 3, embed=False, head=False)
    d2 = str(tmp_path / "qv")
    write_peft(d2, cfg, 8, 16, ("q_proj", "v_proj"), seed=4, use_rslora=True)
    l2 = w2.load_adapters([f"other={d2}"])
    assert l2.names == ["other"] and l2.ranks == {"qkv": 16, "o": 0, "gate_up": 0, "down": 0}
    assert l2.layers[0].o is None and l2.layers[0].gate_up is None and l2.layers[0].down is None
    assert l2.scale[0].item() == np.float32(16 / math.sqrt(8))  # rslora: alpha / sqrt(r)
    assert not bool(l2.layers[0].qkv.B[0, cfg.q_dim:cfg.q_dim + cfg.kv_dim].any())  # the k rows: zero


@pytest.mark.parametrize("field,value", [
    ("use_dora", True), ("modules_to_save", ["lm_head"]), ("rank_pattern", {"q_proj": 4}),
    ("alpha_pattern", {"q_proj": 4}), ("fan_in_fan_out", True), ("target_modules", "q_proj"),
    ("target_modules", ["q_proj", "lm_head"]), ("bias", "all"), ("peft_type", "IA3"), ("r", 65)])
def test_rejected_config_fields_raise_and_are_named(tmp_path, field, value):
    cfg, w = stage_weights(0, 1, head=False)
    d = str(tmp_path / "bad")
    write_peft(d, cfg, 8, 16, ("q_proj",), **{field: value})
    with pytest.raises(ValueError, match=field):
        w.load_adapters([d])


def test_shapes_that_do_not_fit_the_model_raise(tmp_path):
    d = str(tmp_path / "small")
    write_peft(d, resolve_model("small-llama"), 8, 16, ("q_proj",))
    cfg, w = stage_weights(0, 1, head=False)
    with pytest.raises(ValueError, match="shapes"):
        w.load_adapters([d])
    # r <= 64 per module keeps every fused rank within the kernels' 192
    assert ad.fused_rank([(64, ad.MODULES), (8, ("q_proj",))], "qkv") == 192
    with pytest.raises(ValueError, match="exceeds 192"):
        ad.fused_rank([(65, ad.MODULES)], "qkv")


def test_synthetic_adapters_are_deterministic_and_equal_across_stages():
    spec = "synthetic:syn:16"
    assert ad.parse_spec(spec)["modules"] == ("q_proj", "v_proj")
    cfg, full = stage_weights(0, 4)
    _, part = stage_weights(2, 4, embed=False)
    a, b = full.load_adapters([spec]), part.load_adapters([spec])
    for li in (2, 3):
        assert torch.equal(a.layers[li].qkv.A, b.layers[li - 2].qkv.A)
        assert torch.equal(a.layers[li].qkv.B, b.layers[li - 2].qkv.B)
    assert not torch.equal(a.layers[0].qkv.A, a.layers[1].qkv.A)
    _, other = stage_weights(0, 4)
    assert not torch.equal(other.load_adapters(["synthetic:syn2:16"]).layers[0].qkv.A, a.layers[0].qkv.A)
    with pytest.raises(ValueError, match="synthetic"):
        ad.parse_spec("synthetic:x")


# ------------------------------------------------------------------------------------------- torch forms
def _case(M=50, K=384, N=528, R=48, S=4, seed=0):
    g = torch.Generator().manual_seed(seed)
    A = (torch.randn(S, R, K, generator=g) * K ** -0.5).bfloat16()
    B = (torch.randn(S, N, R, generator=g) * R ** -0.5).bfloat16()
    scale = torch.tensor([2.0, 0.5, 1.0, 16 / 8 ** 0.5])
    x = torch.randn(M, K, generator=g).bfloat16()
    y = torch.randn(M, N, generator=g).bfloat16()
    sl = torch.tensor([(0, -1, 3, 1, -1)[(m * 7 + m // 5) % 5] for m in range(M)], dtype=torch.int32)  # slot 2 unused
    return A, B, scale, x, y, sl


def test_torch_forms_within_the_derived_bounds_and_touch_only_their_rows():
    A, B, scale, x, y0, sl = _case()
    M, K = x.shape
    R = A.shape[1]
    nan = float("nan")
    Ap, Bp = A.clone(), B.clone()
    Ap[2], Bp[2] = nan, nan                     # a slot no row names
    xq = x.clone()
    xq[sl < 0] = nan                            # base rows are not read
    t = torch.full((M, R), nan)
    ops.lora_shrink(ops.pack_act(xq), Ap, scale, sl, M, out=t)
    y = y0.clone()
    ops.lora_expand(t, Bp, sl, y)
    live = sl >= 0
    assert bool(torch.isnan(t[~live]).all()) and torch.equal(y[~live], y0[~live])
    idx, s = torch.nonzero(live).flatten(), sl[live].long()
    assert not bool(torch.isnan(t[idx]).any()) and not bool(torch.isnan(y[idx].float()).any())
    prod = A[s].double() * x[idx].double()[:, None, :]
    sc = scale[s].double()[:, None]
    t64 = sc * prod.sum(-1)
    assert bool(((t[idx].double() - t64).abs() <= 2 * K * 2.0 ** -24 * sc * prod.abs().sum(-1)).all())
    bt = B[s].double() * t[idx].double()[:, None, :]
    y64 = y0[idx].double() + bt.sum(-1)
    bound = 2.0 ** -8 * y64.abs() + 2 * (R + 2) * 2.0 ** -24 * (y0[idx].double().abs() + bt.abs().sum(-1))
    assert bool(((y[idx].double() - y64).abs() <= bound).all())
    # the update by runs is the same computation on row-major x
    y2 = y0.clone()
    ops.lora_update(xq, y2, Ap, Bp, scale, ops.lora_runs(sl.tolist()))
    assert torch.equal(y2[~live], y0[~live]) and not bool(torch.isnan(y2.float()).any())
    assert bool(((y2[idx].double() - y64).abs() <= bound + 2 * (R + 2) * 2.0 ** -24 * bt.abs().sum(-1)).all())
    # an all -1 launch changes nothing
    none = torch.full((M,), -1, dtype=torch.int32)
    y3 = y0.clone()
    ops.lora_expand(ops.lora_shrink(ops.pack_act(xq), Ap, scale, none, M), Bp, none, y3)
    assert torch.equal(y3, y0)


def test_torch_forms_row_independence_and_runs():
    A, B, scale, x, y0, sl = _case(seed=1)
    M, m = x.shape[0], 19
    got = []
    for other in (sl, torch.arange(M, dtype=torch.int32) % 4, torch.full((M,), -1, dtype=torch.int32)):
        o = other.clone()
        o[m] = 1
        t = ops.lora_shrink(ops.pack_act(x), A, scale, o, M)
        y = ops.lora_expand(t, B, o, y0.clone())
        got.append((t[m].clone(), y[m].clone()))
    assert all(torch.equal(t, got[0][0]) and torch.equal(y, got[0][1]) for t, y in got[1:])
    assert ops.lora_runs([0, 0, -1, -1, 2, 0, 0]) == [(0, 2, 0), (4, 5, 2), (5, 7, 0)]
    assert ops.lora_runs([-1, -1]) == [] and ops.lora_runs([]) == []
    assert ops.lora_ok(64, 528, 384, 192) and not ops.lora_ok(65, 528, 384, 48) and not ops.lora_ok(4, 528, 384, 208)
    assert not ops.lora_ok(4, 20, 384, 48) and not ops.lora_ok(4, 528, 100, 48) and not ops.lora_ok(4, 528, 384, 24)
    with pytest.raises(ValueError, match="slots"):
        ops.lora_shrink(ops.pack_act(x), A, scale, sl.long(), M)
    with pytest.raises(ValueError, match="t must be"):
        ops.lora_expand(torch.zeros(M, 16), B, sl, y0.clone())


# ------------------------------------------------------------------------------------------- executor
def _executor(peft_dirs, **kw):
    cfg, w = stage_weights()
    w.load_adapters([peft_dirs["a"], peft_dirs["b"]])
    kw.setdefault("max_seq_len", 256)
    return cfg, w, StageExecutor(cfg, w, "cpu", dtype=torch.float32, kv_cache_bytes=32 << 20, max_sessions=8, **kw)


TOL = dict(atol=1e-4, rtol=1e-4)  # the fp32 CPU executor's bound against the oracle (tests/test_executor_cpu.py)


def test_sessions_on_two_adapters_and_none_match_their_merged_oracles(peft_dirs):
    cfg, w, ex = _executor(peft_dirs)
    names = ["a", "b", ""]
    oracle = [[ad.merged_weights(w, ex.adapter_slot(n))] for n in names]
    sids = ["sa", "sb", "s0"]
    g = torch.Generator().manual_seed(0)
    seqs = [torch.randint(0, cfg.vocab_size, (7,), generator=g) for _ in names]
    ex.forward([(s, 7) for s in sids], torch.cat(seqs), adapters=names)
    more = [torch.randint(0, cfg.vocab_size, (5,), generator=g) for _ in names]
    seqs = [torch.cat(p) for p in zip(seqs, more)]
    lg = ex.forward([(s, 5) for s in sids], torch.cat(more), adapters=names)  # prefill 7 + 5 tokens
    for step in range(5):
        for i in range(3):
            ref = reference_forward(oracle[i], seqs[i])[-1]
            torch.testing.assert_close(lg[i], ref, **TOL)
            if names[i]:  # the adapter matters: >= 100 x the bound away from the base model's logits
                assert (ref - reference_forward(oracle[2], seqs[i])[-1]).abs().max().item() >= 100 * TOL["atol"]
        if step == 4:
            break
        nxt = torch.argmax(lg, -1)
        seqs = [torch.cat([s, nxt[i:i + 1]]) for i, s in enumerate(seqs)]
        lg = ex.forward([(s, 1) for s in sids], nxt, adapters=names)
    assert [ex.sessions.get(s).adapter for s in sids] == [0, 1, -1]


def test_chunked_prefill_and_fork_keep_the_adapter(peft_dirs):
    cfg, w, big = _executor(peft_dirs)
    _, _, small = _executor(peft_dirs, max_tokens_per_step=4)
    ids = torch.arange(20) * 13 % cfg.vocab_size
    seqs, names = [("x", 11), ("y", 9)], ["b", "a"]
    ref = big.forward(seqs, ids, reset=[True, True], adapters=names)
    got = small.forward(seqs, ids, reset=[True, True], adapters=names)
    torch.testing.assert_close(got, ref, **TOL)
    torch.testing.assert_close(ref[1], reference_forward([ad.merged_weights(w, 0)], ids[11:])[-1], **TOL)
    # a fork inherits the slot; a step that names no adapters runs every session on its own
    big.sessions.fork("y", "y2")
    assert big.sessions.get("y2").adapter == 0
    nxt = torch.tensor([5])
    torch.testing.assert_close(big.forward([("y2", 1)], nxt), big.forward([("y", 1)], nxt, adapters=["a"]))


def test_adapter_errors(peft_dirs):
    cfg, w, ex = _executor(peft_dirs)
    ids = torch.arange(4)
    ex.forward([("s", 4)], ids, adapters=["a"])
    with pytest.raises(ValueError, match="'a'.*'b'"):
        ex.forward([("s", 1)], ids[:1], adapters=["b"])
    with pytest.raises(ValueError, match="'a'.*''"):
        ex.forward([("s", 1)], ids[:1], adapters=[""])
    ex.forward([("s", 4)], ids, reset=[True], adapters=["b"])  # a reset session may take another one
    with pytest.raises(KeyError, match="adapter nope not found"):
        ex.forward([("t", 4)], ids, adapters=["nope"])
    assert ex.sessions.get("t") is None
    with pytest.raises(ValueError, match="deep prompts"):
        ex.forward([("u", 4)], ids, adapters=["a"], prompts=[torch.zeros(cfg.num_hidden_layers, 2, cfg.hidden_size)])
    _, w0 = stage_weights()
    with pytest.raises(KeyError, match="adapter a not found"):  # a stage without adapters
        StageExecutor(cfg, w0, "cpu", dtype=torch.float32, kv_cache_bytes=8 << 20, max_sessions=2,
                      max_seq_len=64).forward([("s", 4)], ids, adapters=["a"])


def test_combinations_that_are_not_built_raise(peft_dirs):
    spec = ["synthetic:s:8"]
    kw = dict(dtype=torch.float32, kv_cache_bytes=8 << 20, max_sessions=2, max_seq_len=64)
    for quant in ("fp8", "mxfp4"):
        with pytest.raises(ValueError, match="adapters with fp8 or MXFP4"):
            stage_weights(0, 1, head=False, dtype=torch.bfloat16, quant_type=quant)[1].load_adapters(spec)
        with pytest.raises(ValueError, match=f"adapters with {quant}"):
            load_stage_model(MODEL, "cpu", "full", quant_type=quant, adapters=spec)
    with pytest.raises(ValueError, match="adapters with MoE"):
        stage_weights(0, 1, head=False, model="tiny-mixtral")[1].load_adapters(spec)
    with pytest.raises(ValueError, match="adapters with GPT-2"):
        stage_weights(0, 1, head=False, model="tiny-gpt2")[1].load_adapters(spec)
    cfg, w = stage_weights()
    w.load_adapters(spec)
    with pytest.raises(ValueError, match="adapters with tensor parallelism"):
        StageExecutor(cfg, w, "cpu", tp=types.SimpleNamespace(active=True, size=2, capturable=False), **kw)
    with pytest.raises(ValueError, match="adapters with CPU offload"):
        StageExecutor(cfg, w, "cpu", offload=True, **kw)
    with pytest.raises(ValueError, match="adapters with CPU offload"):
        load_stage_model(MODEL, "cpu", "full", use_cpu_offload=True, adapters=spec)
    ops.set_gemm_policy("hipblaslt")  # (conftest puts the policy back)
    with pytest.raises(ValueError, match="adapters with --gemm hipblaslt"):
        StageExecutor(cfg, w, "cpu", **kw)
    ops.set_gemm_policy("auto")
    with pytest.raises(ValueError, match="once per stage"):
        w.load_adapters(spec)


# ------------------------------------------------------------------------------------------- serving surface
def test_rpc_info_and_stateless_requests(peft_dirs):
    cfg = resolve_model(MODEL)
    full = load_stage_model(MODEL, "cpu", "last", start=2, dtype=torch.float32, seed=SEED,
                            adapters=[peft_dirs["a"], f"bee={peft_dirs['b']}"])
    kw = dict(dtype=torch.float32, kv_cache_bytes=8 << 20, max_sessions=2, max_seq_len=64)
    h = StageConnectionHandler(None, StageExecutor(cfg, full.weights, "cpu", **kw), final_stage=True)
    plain = StageConnectionHandler(None, StageExecutor(cfg, stage_weights(2, 4, embed=False)[1], "cpu", **kw),
                                   final_stage=True)
    try:
        assert asyncio.run(h.rpc_info(Message({}, []))).metadata["adapters"] == ["a", "bee"]
        assert "adapters" not in asyncio.run(plain.rpc_info(Message({}, []))).metadata
        hidden = torch.zeros(1, 3, cfg.hidden_size)
        for rpc, ts in ((h.rpc_forward, [hidden]), (h.rpc_backward, [hidden, hidden])):
            with pytest.raises(ValueError, match="stateless.*'bee'"):
                asyncio.run(rpc(Message({"stateless": True, "active_adapter": "bee"}, ts)))
        assert asyncio.run(h.rpc_forward(Message({"stateless": True}, [hidden]))).tensors[0].shape == hidden.shape
    finally:
        h.shutdown()
        plain.shutdown()


def test_adapter_bytes_per_block_and_auto_num_blocks(peft_dirs):
    cfg, w = stage_weights(1, 2, embed=False, head=False)
    specs = [peft_dirs["a"], peft_dirs["b"], "synthetic:s:24:o_proj,down_proj"]
    lora = w.load_adapters(specs)
    per = adapter_bytes_per_block(cfg, specs, torch.float32)
    assert per == lora.nbytes(folded=False) == sum(t.numel() * 4 for t in lora.tensors()) - 4 * len(specs)
    assert adapter_bytes_per_block(cfg, [], torch.float32) == 0
    assert adapter_bytes_per_block(cfg, specs) == per // 2  # bf16 stacks
    block = get_block_size(cfg, "memory", torch.float32) + kv_cache_bytes_per_block(cfg, None, torch.float32)
    free = 40 * block + (2 << 30)
    kw = dict(free_bytes=free, dtype=torch.float32, total_blocks=1000)
    assert auto_num_blocks(cfg, **kw) == 40 == auto_num_blocks(cfg, adapter_bytes=0, **kw)
    assert auto_num_blocks(cfg, adapter_bytes=per, **kw) == (40 * block) // (block + per) < 40


# ------------------------------------------------------------------------------------------- swarm
@pytest.mark.timeout(120)
def test_swarm_with_an_active_adapter_matches_merged_weights(peft_dirs):
    cfg = resolve_model(MODEL)
    host = f"--adapters {peft_dirs['a']} bee={peft_dirs['b']} --dtype fp32 --seed {SEED}"
    s1 = ServerThread(server_argv(MODEL, "2", 1, extra=host)).wait()
    s2 = ServerThread(server_argv(MODEL, "2", 1, peers=s1.addr, extra=f"--dtype fp32 --seed {SEED}")).wait()  # no adapters
    try:
        assert wait_for(lambda: len((s1.dht.get(get_stage_key(1), latest=True) or types.SimpleNamespace(value={}))
                                    .value) == 2)
        recs = {k: (v.value if hasattr(v, "value") else v)
                for k, v in s1.dht.get(get_stage_key(1), latest=True).value.items()}
        assert recs[s1.srv.peer_id]["adapters"] == ["a", "bee"] and "adapters" not in recs[s2.srv.peer_id]
        common = f"--max_new_tokens 6 --temperature 0 --dtype fp32 --seed {SEED} --adapters {peft_dirs['a']} " \
                 f"bee={peft_dirs['b']} --active_adapter "
        _, w = stage_weights()
        lora = w.load_adapters([peft_dirs["a"], f"bee={peft_dirs['b']}"])
        ids = torch.tensor(load_tokenizer(MODEL, cfg).encode("Hello, how are you?"))
        gens = {}
        for name in ("a", "bee"):
            # (every session has to land on the server that hosts the adapter, never on its replica)
            gens[name] = M.run_rank0(client_args(MODEL, "2", s1.addr, common + name), torch.device("cpu"), [2])
            assert gens[name] == greedy_generate([ad.merged_weights(w, lora.slot(name))], ids, len(gens[name]))
        assert gens["bee"] != greedy_generate([ad.merged_weights(w, -1)], ids, len(gens["bee"]))  # not the base model's
        # an adapter the client hosts for its own blocks, but no server does
        other = client_args(MODEL, "2", s1.addr, f"--max_new_tokens 2 --temperature 0 --dtype fp32 --seed {SEED} "
                                                 f"--adapters elsewhere={peft_dirs['b']} --active_adapter elsewhere")
        with pytest.raises(RuntimeError, match="hosts adapter 'elsewhere'"):
            M.run_rank0(other, torch.device("cpu"), [2])
        # ... and one the client itself does not host
        with pytest.raises(KeyError, match="adapter nowhere not found"):
            M.run_rank0(client_args(MODEL, "2", s1.addr, "--active_adapter nowhere"), torch.device("cpu"), [2])
    finally:
        s1.close()
        s2.close()
