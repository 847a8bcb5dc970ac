"""OCP MXFP4 weights (W4A16) on CPU: the quantization rule and the packed layout, ``linear_w4``'s
reference fallback, a 4-bit stage executor, block sizing, and the ``--quant_type`` surface."""
import logging

import pytest
import torch

from src import ops
from src.block_utils import auto_num_blocks, get_block_size
from src.llama_partition import load_stage_model, resolve_quant_type
from src.main import build_parser
from src.models.config import resolve_model
from src.models.reference_model import greedy_generate
from src.models.weights import random_stage_weights
from src.ops import reference as ref
from src.runtime.executor import StageExecutor


def test_mxfp4_pack_unpack_roundtrip():
    torch.manual_seed(0)
    w = torch.randn(96, 512) * 0.02
    w[3] = 0
    w4, s4 = ops.pack_weight_w4(w)
    assert w4.shape == (6, 4, 64, 16) and w4.dtype == torch.uint8
    assert s4.shape == (6, 4, 16, 4) and s4.dtype == torch.uint8
    wd = ops.unpack_weight_w4(w4, s4, torch.float32)
    assert wd.shape == w.shape and torch.isfinite(wd).all()
    assert float(wd[3].abs().max()) == 0.0
    rel = float((wd - w).norm() / w.norm())
    assert rel < 0.125, rel
    assert torch.equal(wd.bfloat16().float(), wd)  # every value is an exact bf16 number
    a4, b4 = ops.pack_weight_w4(wd)  # quantizing the dequantized weight is a fixed point
    assert torch.equal(a4, w4) and torch.equal(b4, s4)
    assert int(s4.min()) >= 1 and int(s4.max()) <= 254
    code, e = ref.unpack_mxfp4(w4, s4)
    assert not bool((code == 0b1000).any())
    assert torch.equal(e[3], torch.ones_like(e[3])) and not bool(code[3].any())  # zero blocks: e = 1, zero codes
    assert torch.equal(ref.unpack_weight_w4(w4, s4, torch.float32), wd)
    with pytest.raises(ValueError):
        ops.pack_weight_w4(torch.zeros(24, 128))
    with pytest.raises(ValueError):
        ops.pack_weight_w4(torch.zeros(16, 96))


def _block(vals):
    """One 32-block (row 0, k 0..31) of a [16, 128] weight -> (codes of the given values, scale byte)."""
    w = torch.zeros(16, 128)
    w[0, : len(vals)] = torch.tensor(vals, dtype=torch.float32)
    code, e = ref.quant_mxfp4(w)
    assert not bool(code[1:].any()) and not bool(code[0, 32:].any())
    assert torch.equal(e.flatten()[1:], torch.ones(16 * 4 - 1, dtype=torch.uint8))
    return code[0, : len(vals)].tolist(), int(e[0, 0])


def test_mxfp4_quantization_edge_cases():
    # amax exactly a power of two: 2^3 -> e = 3 - 2 + 127, scale 2, amax / scale = 4 -> code 6
    assert _block([8.0, 4.0, 2.0, 1.0, 0.0]) == ([6, 4, 2, 1, 0], 128)
    assert _block([2.0 ** -10, 2.0 ** -12]) == ([6, 2], 115)
    # amax = 7.9 x 2^k saturates to 6 (code 7): k = 3 -> floor(log2(63.2)) = 5, e = 130, scale 8
    assert _block([7.9 * 8, -7.9 * 8, 5.5 * 8]) == ([7, 15, 7], 130)
    assert _block([7.9 * 2.0 ** -6]) == ([7], 121)
    # ties (scale 1: amax 4 -> e = 127) round to the even code:
    # 0.25 -> 0 (code 0), 0.75 -> 1 (code 2), 1.25 -> 1 (code 2), 2.5 -> 2 (code 4), 5 -> 4 (code 6)
    assert _block([4.0, 0.25, 0.75, 1.25, 2.5, 5.0]) == ([6, 0, 2, 2, 4, 6], 127)
    # ... and 1.75 -> 2 (code 4), 3.5 -> 4 (code 6); just off a tie goes to the nearer value
    assert _block([4.0, 1.75, 3.5, 0.26, 0.74, 5.01]) == ([6, 4, 6, 1, 1, 7], 127)
    # the same ties at scale 2^-3 (e = 124)
    s = 0.125
    assert _block([4 * s, 0.25 * s, 0.75 * s, 1.25 * s, 2.5 * s, 5 * s]) == ([6, 0, 2, 2, 4, 6], 124)
    # negative values: sign bit 3; a negative value that rounds to zero is +0 (never 0b1000)
    assert _block([-6.0, -0.5, -1.5, -3.0, -0.25, -0.1, 3.0]) == ([15, 9, 11, 13, 0, 0, 5], 127)
    # dequantization: code value x 2^(e - 127)
    code = torch.tensor([[6, 15, 1, 9] + [0] * 124] + [[0] * 128] * 15, dtype=torch.uint8)
    e = torch.full((16, 4), 127, dtype=torch.uint8)
    e[0, 0] = 130
    assert ref.dequant_mxfp4(code, e)[0, :5].tolist() == [32.0, -48.0, 4.0, -4.0, 0.0]
    # nibble and byte order of the packed layout: lower k in the low nibble, lane = 16 (k/8 % 4) + row
    w4, s4 = ref.pack_mxfp4(code, e)
    assert w4[0, 0, 0, :2].tolist() == [6 | (15 << 4), 1 | (9 << 4)] and int(w4.sum()) == 0x6 + 0xF0 + 0x1 + 0x90
    assert s4[0, 0, 0].tolist() == [130, 127, 127, 127]


@pytest.mark.parametrize("M", [5, 21])
def test_linear_w4_cpu_matches_dequantized_product(M):
    torch.manual_seed(1 + M)
    K, N = 512, 64
    x = torch.randn(M, K).bfloat16()
    xp = ref.pack_act(x)
    w4, s4 = ops.pack_weight_w4(torch.randn(N, K) * 0.02)
    wd = ops.unpack_weight_w4(w4, s4, torch.float32)
    exact = x.float() @ wd.t()
    # epilogue 0
    y = ops.linear_w4(xp, w4, s4, M)
    torch.testing.assert_close(y.float(), exact, atol=2e-3, rtol=1e-2)
    # epilogue 0 with the fused-norm row scale
    ss = ops.norm_stats_buffer("cpu")[0]
    ss[0, :M] = ref.fx_sumsq(x)
    y = ops.linear_w4(xp, w4, s4, M, ss_in=ss, eps=1e-5)
    rs = torch.rsqrt(x.float().pow(2).mean(-1, keepdim=True) + 1e-5)
    torch.testing.assert_close(y.float(), exact * rs, atol=2e-3, rtol=1e-2)
    # epilogue 1: packed SwiGLU of a 16-row interleaved gate/up weight
    g4, gs4 = ops.pack_weight_w4(torch.randn(2 * N, K) * 0.02)
    gd = ops.unpack_weight_w4(g4, gs4, torch.float32)
    act = ops.linear_w4(xp, g4, gs4, M, epilogue=1, out_packed=True)
    want = ref.swiglu((x.float() @ gd.t()).bfloat16()).float()
    torch.testing.assert_close(ref.unpack_act(act, M, N).float(), want, atol=2e-3, rtol=1e-2)
    # epilogue 3: residual-stream producer
    r = torch.randn(M, N).bfloat16()
    r0 = r.clone()
    ap = torch.zeros(ops.packed_numel(M, N), dtype=torch.bfloat16)
    sso, ssz = ops.norm_stats_buffer("cpu")[0], ops.norm_stats_buffer("cpu")[0] + 5
    out = ops.linear_w4(xp, w4, s4, M, out=r, epilogue=3, residual=r, ap_out=ap, ss_out=sso, ss_zero=ssz)
    assert out is r
    want = (r0.float() + exact.bfloat16().float()).bfloat16()
    torch.testing.assert_close(r.float(), want.float(), atol=2e-3, rtol=1e-2)
    assert torch.equal(ref.unpack_act(ap, M, N), r)
    assert torch.equal(sso.sum(0)[:M], ref.fx_sumsq(r)) and int(ssz.abs().sum()) == 0


def _stage(cfg, device, dtype, seed=0):
    return random_stage_weights(cfg, 0, cfg.num_hidden_layers, has_embed=True, has_head=True, device=device,
                                dtype=dtype, seed=seed)


def test_mxfp4_stage_executor_matches_dequantized_reference():
    cfg = resolve_model("small-llama")
    w, wd = _stage(cfg, "cpu", torch.float32), _stage(cfg, "cpu", torch.float32)
    gn = torch.Generator().manual_seed(11)
    for L in w.layers:  # non-unit norms, set before the quantization folds them in
        L.input_norm = 0.5 + torch.rand(cfg.hidden_size, generator=gn)
        L.post_norm = 0.5 + torch.rand(cfg.hidden_size, generator=gn)
    w.quantize_mxfp4(drop_dense=True)
    assert w.w4 and not w.fp8 and w.layers[0].qkv is None and w.layers[0].folded
    # the oracle: the dequantized (folded) weights with unit norms
    for L, Ld in zip(w.layers, wd.layers):
        for name in L.PROJ:
            setattr(Ld, name, L.dense(name, torch.float32))
        assert torch.equal(Ld.input_norm, torch.ones(cfg.hidden_size))
    ids = torch.randint(0, cfg.vocab_size, (12,), generator=torch.Generator().manual_seed(3))
    want = greedy_generate([wd], ids, 6)
    ex = StageExecutor(cfg, w, "cpu", dtype=torch.float32, kv_cache_bytes=16 << 20, max_sessions=2, max_seq_len=64)
    assert ex.quant_type == "mxfp4" and not ex._w4  # (the W4A16 kernels are the GPU path)
    logits = ex.forward([("s", len(ids))], ids, reset=[True])
    got = [int(torch.argmax(logits[-1]))]
    for _ in range(5):
        logits = ex.forward([("s", 1)], torch.tensor([got[-1]]))
        got.append(int(torch.argmax(logits[-1])))
    assert got == want


def test_mxfp4_unsupported_configurations_raise():
    moe = resolve_model("tiny-mixtral")
    with pytest.raises(ValueError, match="MoE"):
        random_stage_weights(moe, 0, 1, has_embed=False, has_head=False, device="cpu", quant_type="mxfp4")
    with pytest.raises(ValueError):
        random_stage_weights(resolve_model("tiny-llama"), 0, 1, has_embed=False, has_head=False, device="cpu",
                             quant_type="int3")
    with pytest.raises(ValueError, match="offload"):
        load_stage_model("tiny-llama", "cpu", "full", quant_type="mxfp4", use_cpu_offload=True)
    # the fp8= keyword keeps working, and agrees with quant_type="fp8"
    cfg = resolve_model("tiny-llama")
    a = random_stage_weights(cfg, 0, 1, has_embed=False, has_head=False, device="cpu", fp8=True)
    b = random_stage_weights(cfg, 0, 1, has_embed=False, has_head=False, device="cpu", quant_type="fp8")
    assert a.fp8 and b.fp8 and not a.w4 and torch.equal(a.layers[0].qkv_q, b.layers[0].qkv_q)


def test_block_size_and_auto_num_blocks_for_mxfp4():
    cfg = resolve_model("llama2-7b")
    H = cfg.hidden_size
    matrices = cfg.layer_param_bytes(1.0) - 2 * H
    norms = 2 * H * 2
    size = get_block_size(cfg, "memory", torch.bfloat16, "mxfp4")
    assert size == int(matrices * 4.25 / 8 + norms)
    fp8 = get_block_size(cfg, "memory", torch.bfloat16, "fp8")
    assert size < fp8 < get_block_size(cfg, "memory", torch.bfloat16)
    assert get_block_size(cfg, "memory", torch.bfloat16, "nf4") == size
    free = 6 << 30  # (small enough that neither count is clamped to the 32 blocks)
    n4 = auto_num_blocks(cfg, free_bytes=free, quant_type="mxfp4", attn_cache_tokens=2048)
    n8 = auto_num_blocks(cfg, free_bytes=free, quant_type="fp8", attn_cache_tokens=2048)
    assert n4 > n8 >= 1, (n4, n8)


def test_quant_type_parser_and_loader(caplog):
    argv = ["--model", "tiny-llama", "--splits", "1", "--stage", "1"]
    assert build_parser().parse_args(argv).quant_type == "none"
    args = build_parser().parse_args(argv + ["--quant_type", "nf4"])
    assert args.quant_type == "nf4"
    with pytest.raises(SystemExit):
        build_parser().parse_args(argv + ["--quant_type", "int3"])
    with caplog.at_level(logging.INFO, logger="src.llama_partition"):
        assert resolve_quant_type(args.quant_type) == "mxfp4"
    assert "nf4" in caplog.text and "using mxfp4" in caplog.text
    caplog.clear()
    with caplog.at_level(logging.INFO, logger="src.llama_partition"):
        assert resolve_quant_type("int8") == "fp8"
    assert "int8" in caplog.text and "using fp8" in caplog.text
    assert [resolve_quant_type(q) for q in (None, "none", "fp8", "mxfp4")] == ["none", "none", "fp8", "mxfp4"]
    with pytest.raises(ValueError):
        resolve_quant_type("int3")
    full = load_stage_model("tiny-llama", "cpu", "full", quant_type="mxfp4")
    assert full.weights.w4 and full.weights.layers[0].qkv is None and full.weights.layers[0].qkv_w4 is not None
    assert load_stage_model("tiny-llama", "cpu", "full", quant_type="int8").weights.fp8
    assert not load_stage_model("tiny-llama", "cpu", "full").weights.w4
    with pytest.raises(ValueError):
        load_stage_model("tiny-mixtral", "cpu", "full", quant_type="mxfp4")


@pytest.mark.timeout(120)
def test_stage_server_with_quant_type_generates_and_announces_it():
    """``--quant_type nf4`` on a stage server (CPU): the client's tokens equal greedy decoding over
    the unquantized first stage + the dequantized MXFP4 blocks; ``rpc_info`` and the stage's
    announcement carry ``quant_type: mxfp4``."""
    from src import main as M
    from src.comm.wire import Message
    from src.dht_utils import get_stage_key
    from src.models.tokenizer import load_tokenizer

    from .swarm_utils import ServerThread, client_args, server_argv

    model, cut = "tiny-llama", 2
    cfg = resolve_model(model)
    s1 = ServerThread(server_argv(model, str(cut), 1, extra="--quant_type nf4")).wait()
    try:
        assert s1.srv.ex.quant_type == "mxfp4" and s1.srv.ex.w.w4
        info = s1.srv.loop.run(s1.srv.handler.rpc_info(Message({}, [])), timeout=10)
        assert info.metadata["quant_type"] == "mxfp4"
        rec = s1.dht.get(get_stage_key(1), latest=True)
        assert "mxfp4" in repr(rec.value)
        args = client_args(model, str(cut), s1.addr, "--max_new_tokens 6 --temperature 0")
        gen = M.run_rank0(args, torch.device("cpu"), [cut])
    finally:
        s1.close()
    wd = _stage(cfg, "cpu", torch.float32)
    for L in wd.layers[cut:]:
        for name in L.PROJ:
            setattr(L, name, ops.unpack_weight_w4(*ops.pack_weight_w4(getattr(L, name)), torch.float32))
    ids = torch.tensor(load_tokenizer(model, cfg).encode("Hello, how are you?"))
    assert gen == greedy_generate([wd], ids, len(gen)) and len(gen) == 6
