"""MXFP4 (W4A16) on the GPU: the HIP dequantizer bit for bit against the torch reference, the
ring GEMM (ops/csrc/gemm_w4.hip) with the three fused-norm epilogues against fp32 oracles on the
dequantized weights, and a 4-bit stage executor (fused-norm decode, dense path, > 64 rows)."""
import pytest
import torch

from src import ops
from src.models.config import resolve_model
from src.models.reference_model import reference_forward
from src.models.weights import random_stage_weights
from src.ops import reference as ref
from src.runtime.executor import StageExecutor

EPS = 1e-5
BF = torch.bfloat16


def _weights(N, K, dev, g, gw=None):
    """Random weight (norm weight ``gw`` folded along K before the one quantization) ->
    (w4, s4, dequantized fp32 [N, K])."""
    w = torch.randn(N, K, device=dev, generator=g) * 0.03
    if gw is not None:
        w = w * gw.float()[None, :]
    w4, s4 = ops.pack_weight_w4(w)
    return w4, s4, ref.unpack_weight_w4(w4, s4, torch.float32)


@pytest.mark.gpu
@pytest.mark.parametrize("K", [128, 640])
@pytest.mark.parametrize("N", [16, 48, 256])
def test_dequantizer_equals_reference_bit_for_bit(N, K):
    """Every emitted code, scale bytes over the whole range (1 and 254 included): pins the nibble
    order, the byte-select order and the hardware convert."""
    dev = "cuda"
    g = torch.Generator(device=dev).manual_seed(N * 1000 + K)
    code = torch.randint(0, 16, (N, K), device=dev, generator=g, dtype=torch.uint8)
    code[code == 8] = 0  # negative zero is never emitted
    code[1, :16] = torch.arange(16, device=dev, dtype=torch.uint8)
    code[1, 8] = 0
    e = torch.randint(1, 255, (N, K // 32), device=dev, generator=g, dtype=torch.uint8)
    e[0, 0], e[0, 1], e[1, 0], e[2, 0], e[3, 0] = 1, 254, 127, 2, 253
    assert set(code.unique().tolist()) == set(range(16)) - {8}
    assert int(e.min()) == 1 and int(e.max()) == 254
    w4, s4 = ref.pack_mxfp4(code, e)
    assert w4.shape == (N // 16, K // 128, 64, 16) and s4.shape == (N // 16, K // 128, 16, 4)
    want = ref.unpack_weight_w4(w4, s4, BF)
    got = ops.unpack_weight_w4(w4, s4, BF)
    assert got.dtype == BF and got.shape == (N, K)
    assert torch.equal(got.view(torch.int16), want.view(torch.int16))  # bit for bit (signed zeros, inf included)
    assert torch.equal(want.cpu().view(torch.int16), ref.unpack_weight_w4(w4.cpu(), s4.cpu(), BF).view(torch.int16))


@pytest.mark.gpu
@pytest.mark.parametrize("N", [256, 2048])
@pytest.mark.parametrize("K", [512, 1152, 2048])
@pytest.mark.parametrize("M", [1, 13, 16, 17, 50, 64])
def test_w4a16_gemm_epilogues_match_fp32_oracle(M, K, N):
    """Oracle: x.float() @ dequant(W).float().t().  Every row-tile count and partial tiles (M),
    an uneven split of the 128-deep steps over the 4 waves (K = 1152: 9 steps), one or several
    column tiles per workgroup (N)."""
    dev = "cuda"
    g = torch.Generator(device=dev).manual_seed(M * 100000 + K * 10 + N)
    for epi, n in ((0, N), (1, 2 * N), (3, N)):
        assert ops.w4_gemm_ok(M, n, K, epi), (M, n, K, epi)
    x = (torch.randn(M, K, device=dev, generator=g) * 0.7).to(BF)
    gw = (torch.rand(K, device=dev, generator=g) + 0.5).to(BF)
    # the stage-entry norm kernel: raw x packed + its row statistics
    ss = ops.norm_stats_buffer(dev)[0] + 3
    res = torch.empty_like(x)
    xp = torch.zeros(ops.packed_numel(M, K), dtype=BF, device=dev)
    ops.rmsnorm(x, gw, EPS, out=xp, residual=res, mode=3, packed=True, ss=ss)
    xn = x.float() * torch.rsqrt(x.float().pow(2).mean(-1, keepdim=True) + EPS)

    # epilogue 0 with the ss_in row scale
    w4, s4, wd = _weights(N, K, dev, g, gw)
    y = ops.linear_w4(xp, w4, s4, M, ss_in=ss, eps=EPS)
    assert y.shape == (M, N)
    torch.testing.assert_close(y.float(), xn @ wd.t(), atol=3e-2, rtol=3e-2)

    # epilogue 1: packed SwiGLU of a 16-row interleaved gate/up weight
    g4, gs4, gd = _weights(2 * N, K, dev, g, gw)
    act = torch.zeros(ops.packed_numel(M, N), dtype=BF, device=dev)
    ops.linear_w4(xp, g4, gs4, M, out=act, epilogue=1, out_packed=True, ss_in=ss, eps=EPS)
    exp = ref.swiglu((xn @ gd.t()).to(BF)).float()
    torch.testing.assert_close(ref.unpack_act(act, M, N).float(), exp, atol=5e-2, rtol=3e-2)

    # epilogue 3: residual-stream producer
    a = (torch.randn(M, K, device=dev, generator=g) * 0.5).to(BF)
    o4, os4, od = _weights(N, K, dev, g)
    r = torch.randn(M, N, device=dev, generator=g).to(BF)
    r0 = r.clone()
    ap = torch.zeros(ops.packed_numel(M, N), dtype=BF, device=dev)
    sso, ssz = ops.norm_stats_buffer(dev)[0], ops.norm_stats_buffer(dev)[0] + 7
    ops.linear_w4(ops.pack_act(a), o4, os4, M, out=r, epilogue=3, residual=r, ap_out=ap, ss_out=sso, ss_zero=ssz)
    exp = (r0.float() + (a.float() @ od.t()).to(BF).float()).to(BF)
    torch.testing.assert_close(r.float(), exp.float(), atol=2e-2, rtol=2e-2)
    assert torch.equal(ref.unpack_act(ap, M, N), r)
    assert torch.equal(sso.sum(0)[:M].cpu(), ref.fx_sumsq(r.cpu()))
    assert int(ssz.abs().sum()) == 0


@pytest.mark.gpu
@pytest.mark.parametrize("M", [13, 50])
def test_padding_rows_of_a_partial_tile_are_never_read_into_the_result(M):
    """NaN in the packed activation rows past M (last 16-row tile): rows below M unchanged, finite."""
    dev = "cuda"
    g = torch.Generator(device=dev).manual_seed(7000 + M)
    K, N = 1152, 256
    MT = (M + 15) // 16
    x = (torch.randn(MT * 16, K, device=dev, generator=g) * 0.7).to(BF)
    x[M:] = 0
    clean = ref.pack_act(x)
    x[M:] = float("nan")
    dirty = ref.pack_act(x)
    assert clean.numel() == ops.packed_numel(M, K) and bool(torch.isnan(dirty.float()).any())
    w4, s4, wd = _weights(N, K, dev, g)
    g4, gs4, _ = _weights(2 * N, K, dev, g)
    y0, y1 = ops.linear_w4(clean, w4, s4, M), ops.linear_w4(dirty, w4, s4, M)
    assert torch.isfinite(y1.float()).all() and torch.equal(y0, y1)
    torch.testing.assert_close(y1.float(), x[:M].float() @ wd.t(), atol=3e-2, rtol=3e-2)
    a0, a1 = (ops.linear_w4(p, g4, gs4, M, epilogue=1, out_packed=True) for p in (clean, dirty))
    u0, u1 = ref.unpack_act(a0, M, N), ref.unpack_act(a1, M, N)
    assert torch.isfinite(u1.float()).all() and torch.equal(u0, u1)


# ------------------------------------------------------------------ stage executor
@pytest.fixture(scope="module")
def w4_stage():
    """small-llama with non-unit norms quantized to MXFP4, and the fp32 oracle weights: the
    dequantized (norm-folded) projections with unit norms.  Built once, never modified by a test."""
    cfg = resolve_model("small-llama")
    n = cfg.num_hidden_layers
    w = random_stage_weights(cfg, 0, n, has_embed=True, has_head=True, device="cuda", seed=5)
    wd = random_stage_weights(cfg, 0, n, has_embed=True, has_head=True, device="cuda", seed=5, dtype=torch.float32)
    gn = torch.Generator(device="cuda").manual_seed(11)
    for L in w.layers:
        for nm in ("input_norm", "post_norm"):
            setattr(L, nm, (0.5 + torch.rand(cfg.hidden_size, device="cuda", generator=gn)).to(BF))
    w.quantize_mxfp4(drop_dense=True)
    assert w.w4 and w.layers[0].qkv is None
    for L, Ld in zip(w.layers, wd.layers):
        for name in L.PROJ:
            setattr(Ld, name, ref.unpack_weight_w4(getattr(L, name + "_w4"), getattr(L, name + "_s4"), torch.float32))
    return cfg, w, wd


def _decode(ex, cfg, n, n_steps):
    """Ragged prefill of ``n`` sessions, then ``n_steps`` decode steps -> (logits per step, token rows)."""
    prompts = [torch.randint(0, cfg.vocab_size, (5 + i % 7,), generator=torch.Generator().manual_seed(i))
               for i in range(n)]
    seqs = [(f"s{i}", len(p)) for i, p in enumerate(prompts)]
    ex.forward(seqs, torch.cat(prompts).cuda(), reset=[True] * n)
    cur = [p.clone() for p in prompts]
    steps = []
    for _ in range(n_steps):
        tok = torch.tensor([int(c[-1]) * 7 % cfg.vocab_size for c in cur])
        cur = [torch.cat([c, tok[i:i + 1]]) for i, c in enumerate(cur)]
        steps.append(ex.forward([(s, 1) for s, _ in seqs], tok.cuda()).float())
    return steps, cur


def _check_oracle(wd, steps, cur, rows):
    for i in rows:
        want = reference_forward([wd], cur[i].cuda())[-1].float()
        cos = torch.nn.functional.cosine_similarity(steps[-1][i], want, dim=0)
        assert float(cos) > 0.99, (i, float(cos))


@pytest.mark.gpu
@pytest.mark.parametrize("fused", [True, False])
@pytest.mark.parametrize("graphs", [False, True])
def test_mxfp4_executor_decode_tracks_dequantized_oracle(w4_stage, graphs, fused, monkeypatch):
    """17 ragged sessions, prefill + 3 decode steps on the fused-norm W4A16 path (or, with
    MPAMD_FUSED_NORM=0, the dequantizing dense path), with and without hipGraphs (bit for bit)."""
    cfg, w, wd = w4_stage
    if not fused:
        monkeypatch.setenv("MPAMD_FUSED_NORM", "0")
    calls = []
    real = ops.linear_w4
    monkeypatch.setattr(ops, "linear_w4", lambda *a, **k: (calls.append(1), real(*a, **k))[1])
    outs = {}
    for g in sorted({False, graphs}):
        ex = StageExecutor(cfg, w, "cuda", kv_cache_bytes=64 << 20, max_sessions=32, max_seq_len=128, use_graphs=g)
        assert ex._w4 and ex._fused == fused and ex.quant_type == "mxfp4"
        assert ex._w4_ok(17) and not ex._qkv_fold(17)
        outs[g] = _decode(ex, cfg, 17, 3)
    assert bool(calls) == fused  # 4 W4A16 GEMMs per layer and step on the fused path, none on the dense one
    steps, cur = outs[graphs]
    if graphs:
        for a, b in zip(outs[False][0], steps):
            assert torch.equal(a, b)
    _check_oracle(wd, steps, cur, (0, 5, 16))


@pytest.mark.gpu
def test_mxfp4_executor_65_sessions_take_the_dequantizing_path(w4_stage, monkeypatch):
    """A 65-row decode step is past the W4A16 kernel's 64 rows: LlamaLayer.dense() + the HIP dequantizer."""
    cfg, w, wd = w4_stage
    gemm, deq = [], []
    real_l, real_u = ops.linear_w4, ops.unpack_weight_w4
    monkeypatch.setattr(ops, "linear_w4", lambda *a, **k: (gemm.append(1), real_l(*a, **k))[1])
    monkeypatch.setattr(ops, "unpack_weight_w4", lambda *a, **k: (deq.append(a[0].is_cuda), real_u(*a, **k))[1])
    ex = StageExecutor(cfg, w, "cuda", kv_cache_bytes=128 << 20, max_sessions=80, max_seq_len=64, use_graphs=False)
    assert ex._w4 and ex._fused and not ex._w4_ok(65)
    steps, cur = _decode(ex, cfg, 65, 1)
    assert not gemm and deq and all(deq)
    assert steps[-1].shape[0] == 65 and torch.isfinite(steps[-1]).all()
    _check_oracle(wd, steps, cur, (0, 5, 16, 64))
