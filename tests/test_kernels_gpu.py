"""Numerics of every gfx950 HIP kernel against a plain-PyTorch fp32 reference of the same op."""
import math

import numpy as np
import pytest
import torch

from src import ops
from src.ops import reference as ref

pytestmark = pytest.mark.gpu
DEV = "cuda"


@pytest.fixture(scope="module", autouse=True)
def _native():
    assert ops.load_library(), "HIP kernel library must load on the GPU box"
    torch.manual_seed(0)


def bf(x):
    return x.to(torch.bfloat16)


@pytest.mark.parametrize("H", [256, 4096, 8192, 768])
@pytest.mark.parametrize("mode", [0, 1, 2])
def test_rmsnorm(H, mode):
    T = 37
    x = bf(torch.randn(T, H, device=DEV))
    w = bf(torch.rand(H, device=DEV) + 0.5)
    res = bf(torch.randn(T, H, device=DEV))
    res_ref = res.clone()
    y = ops.rmsnorm(x, w, 1e-5, residual=res, mode=mode)
    yr = ref.rmsnorm(x.cpu(), w.cpu(), 1e-5, residual=res_ref.cpu() if mode else None, mode=mode)
    torch.testing.assert_close(y.cpu().float(), yr.float(), atol=2e-2, rtol=2e-2)
    if mode == 1:
        torch.testing.assert_close(res.cpu().float(), (res_ref.float() + x.float()).cpu(), atol=3e-2, rtol=1e-2)
    if mode == 2:
        assert torch.equal(res, x)
    # fp32 oracle
    src = (res_ref.float() + x.float()) if mode == 1 else x.float()
    o = src * torch.rsqrt(src.pow(2).mean(-1, keepdim=True) + 1e-5) * w.float()
    torch.testing.assert_close(y.float(), o, atol=5e-2, rtol=3e-2)


def test_rmsnorm_rows():
    x = bf(torch.randn(20, 512, device=DEV))
    w = bf(torch.rand(512, device=DEV))
    rows = torch.tensor([3, 19, 0], dtype=torch.int32, device=DEV)
    y = ops.rmsnorm(x, w, 1e-6, rows=rows)
    yr = ref.rmsnorm(x[rows.long()], w, 1e-6)
    torch.testing.assert_close(y, yr, atol=1e-2, rtol=1e-2)


def _make_cache(P, nkv, ps, D):
    k = bf(torch.randn(P, nkv, ps, D, device=DEV))
    v = bf(torch.randn(P, nkv, ps, D, device=DEV))
    return k, v


@pytest.mark.parametrize("nh,nkv,D", [(32, 32, 128), (8, 2, 128), (12, 12, 64), (64, 8, 128)])
def test_rope_kv_write(nh, nkv, D):
    T, P, ps = 19, 16, 64
    qkv = bf(torch.randn(T, (nh + 2 * nkv) * D, device=DEV))
    pos = torch.randint(0, 1000, (T,), device=DEV)
    slots = torch.randperm(P * ps, device=DEV)[:T]
    slots[3] = -1
    cos, sin = ops.rope_cos_sin(D, 2048, 10000.0, DEV)
    kc, vc = _make_cache(P, nkv, ps, D)
    kr, vr, qr = kc.clone(), vc.clone(), qkv.clone()
    ops.rope_kv_write(qkv, pos, cos, sin, kc, vc, slots, nh, nkv)
    ref.rope_kv_write(qr, pos, cos, sin, kr, vr, slots, nh, nkv)
    torch.testing.assert_close(qkv.float(), qr.float(), atol=2e-2, rtol=1e-2)
    torch.testing.assert_close(kc.float(), kr.float(), atol=2e-2, rtol=1e-2)
    assert torch.equal(vc, vr)


def _attn_case(nh, nkv, D, ctxs, ps=64, multi_q=False):
    S = len(ctxs)
    maxp = max(math.ceil(c / ps) for c in ctxs) + 1
    P = S * maxp + 3
    kc, vc = _make_cache(P, nkv, ps, D)
    perm = torch.randperm(P, device=DEV)[: S * maxp].view(S, maxp).to(torch.int32)
    if multi_q:  # every position of every sequence is a query (prefill-as-decode, causal)
        q_seq = torch.cat([torch.full((c,), i, dtype=torch.int32) for i, c in enumerate(ctxs)]).to(DEV)
        q_ctx = torch.cat([torch.arange(1, c + 1, dtype=torch.int32) for c in ctxs]).to(DEV)
    else:
        q_seq = torch.arange(S, dtype=torch.int32, device=DEV)
        q_ctx = torch.tensor(ctxs, dtype=torch.int32, device=DEV)
    T = q_seq.numel()
    q = bf(torch.randn(T, (nh + 2 * nkv) * D, device=DEV))  # strided q view like the executor's qkv
    return q, kc, vc, perm, q_seq, q_ctx


@pytest.mark.parametrize("nh,nkv,D", [(32, 32, 128), (32, 8, 128), (64, 8, 128), (16, 8, 128), (12, 12, 64),
                                      (8, 2, 64)])
@pytest.mark.parametrize("ctxs", [[1, 5, 64, 200], [1000, 3], [4097], [150] * 40])
def test_paged_attention_decode(nh, nkv, D, ctxs):
    q, kc, vc, bt, q_seq, q_ctx = _attn_case(nh, nkv, D, ctxs)
    scale = 1 / math.sqrt(D)
    out = ops.paged_attention(q, kc, vc, bt, q_seq, q_ctx, nh, nkv, scale)
    o_ref = ref.paged_attention(q.float(), kc.float(), vc.float(), bt, q_seq, q_ctx, nh, nkv, scale)
    torch.testing.assert_close(out.float(), o_ref.float(), atol=2e-2, rtol=2e-2)


@pytest.mark.parametrize("parts", [(64, 1), (64, 8), (128, 4), (2048, 1)])
def test_paged_attention_explicit_partitions(parts):
    nh, nkv, D = 32, 8, 128
    q, kc, vc, bt, q_seq, q_ctx = _attn_case(nh, nkv, D, [300, 17, 1])
    ps, np_ = parts
    if ps * np_ < 300:
        np_ = math.ceil(300 / ps)
    out = ops.paged_attention(q, kc, vc, bt, q_seq, q_ctx, nh, nkv, 0.088, part_size=ps, num_parts=np_)
    o_ref = ref.paged_attention(q.float(), kc.float(), vc.float(), bt, q_seq, q_ctx, nh, nkv, 0.088)
    torch.testing.assert_close(out.float(), o_ref.float(), atol=2e-2, rtol=2e-2)


@pytest.mark.parametrize("packed", [False, True])
@pytest.mark.parametrize("ctxs,parts", [([300, 17, 1, 0], (64, 5)), ([150], (64, 3)), ([4097, 2], (128, 33))])
def test_paged_attention_inlaunch_combine_equals_reduce_kernel(ctxs, parts, packed, monkeypatch):
    """The in-launch split-K combine (last-arriving slice sums the partials) gives exactly the
    separate reduce kernel's output (same arithmetic, slice order), with empty slices (short
    contexts, ctx = 0 rows) arriving too; the counters are left at zero for the next launch."""
    nh, nkv, D = 32, 8, 128
    q, kc, vc, bt, q_seq, q_ctx = _attn_case(nh, nkv, D, ctxs)
    ps, np_ = parts
    outs = []
    for flag in ("0", "1", "1"):
        monkeypatch.setattr(ops, "ATTN_INLAUNCH_REDUCE", flag == "1")
        outs.append(ops.paged_attention(q, kc, vc, bt, q_seq, q_ctx, nh, nkv, 0.088, part_size=ps, num_parts=np_,
                                        packed=packed))
    torch.cuda.synchronize()
    if packed:  # padding rows of the last 16-row tile are never written: compare the real rows
        outs = [ops.unpack_act(o, len(ctxs), nh * D) for o in outs]
    assert torch.equal(outs[0], outs[1]) and torch.equal(outs[1], outs[2])
    assert int(ops.attention_counters(DEV).abs().sum()) == 0
    o_ref = ref.paged_attention(q.float(), kc.float(), vc.float(), bt, q_seq, q_ctx, nh, nkv, 0.088)
    torch.testing.assert_close(outs[1].float(), o_ref.float(), atol=2e-2, rtol=2e-2)


def test_paged_attention_prefill_causal_and_padding():
    nh, nkv, D = 16, 4, 128
    q, kc, vc, bt, q_seq, q_ctx = _attn_case(nh, nkv, D, [70, 9], multi_q=True)
    q_ctx[5] = 0  # padded row -> zeros
    out = ops.paged_attention(q, kc, vc, bt, q_seq, q_ctx, nh, nkv, 0.1)
    o_ref = ref.paged_attention(q.float(), kc.float(), vc.float(), bt, q_seq, q_ctx, nh, nkv, 0.1)
    torch.testing.assert_close(out.float(), o_ref.float(), atol=2e-2, rtol=2e-2)
    assert out[5].abs().max().item() == 0


def test_paged_attention_spike_forces_rescale():
    """One huge K row makes a single partition dominate: exercises the split-K combine."""
    nh, nkv, D = 8, 8, 128
    q, kc, vc, bt, q_seq, q_ctx = _attn_case(nh, nkv, D, [1500])
    page = int(bt[0, 10])
    kc[page, :, 5, :] = q[0, : nh * D].view(nh, D)[::1][:nkv] * 8
    out = ops.paged_attention(q, kc, vc, bt, q_seq, q_ctx, nh, nkv, 1 / math.sqrt(D), part_size=64, num_parts=24)
    o_ref = ref.paged_attention(q.float(), kc.float(), vc.float(), bt, q_seq, q_ctx, nh, nkv, 1 / math.sqrt(D))
    torch.testing.assert_close(out.float(), o_ref.float(), atol=2e-2, rtol=2e-2)


def test_swiglu_add_embedding_argmax():
    T, F = 33, 11008
    gu = bf(torch.randn(T, 2 * F, device=DEV))
    torch.testing.assert_close(ops.swiglu(gu).float(), ref.swiglu(gu.cpu()).float().to(DEV), atol=1e-2, rtol=1e-2)
    a, b = bf(torch.randn(T, 4096, device=DEV)), bf(torch.randn(T, 4096, device=DEV))
    assert torch.equal(ops.add(a, b), (a.float() + b.float()).to(torch.bfloat16))
    table = bf(torch.randn(1000, 4096, device=DEV))
    ids = torch.randint(0, 1000, (T,), device=DEV)
    assert torch.equal(ops.embedding(ids, table), table[ids])
    logits = bf(torch.randn(T, 32000, device=DEV))
    logits[3, 7] = 100
    logits[3, 9] = 100  # tie -> first index
    am = ops.argmax(logits)
    assert torch.equal(am, torch.argmax(logits.float(), -1))
    assert am[3].item() == 7


@pytest.mark.parametrize("M", [1, 7, 16, 33, 64])
@pytest.mark.parametrize("N,K", [(4096, 4096), (12288, 4096), (4096, 11008), (768, 768), (8192, 384), (32000, 4096)])
def test_gemm_native(M, N, K):
    x = bf(torch.randn(M, K, device=DEV))
    w = bf(torch.randn(N, K, device=DEV) * 0.02)
    wp = ops.pack_weight(w)
    assert torch.equal(ops.unpack_weight(wp), w)
    assert torch.equal(wp.cpu(), ops.pack_weight(w.cpu()))
    y = ops.linear(x, None, policy="native", wp=wp)
    yr = (x.float() @ w.float().t())
    torch.testing.assert_close(y.float(), yr, atol=3e-2, rtol=2e-2)


@pytest.mark.parametrize("M", [1, 40, 64])
def test_gemm_swiglu_and_residual_epilogues(M):
    K, F = 4096, 1024
    x = bf(torch.randn(M, K, device=DEV))
    gate = bf(torch.randn(F, K, device=DEV) * 0.02)
    up = bf(torch.randn(F, K, device=DEV) * 0.02)
    from src.models.weights import interleave_gate_up

    gu = interleave_gate_up(gate, up)
    y = ops.linear(x, gu, epilogue=1, policy="native", wp=ops.pack_weight(gu))
    g, u = x.float() @ gate.float().t(), x.float() @ up.float().t()
    torch.testing.assert_close(y.float(), torch.nn.functional.silu(g) * u, atol=3e-2, rtol=3e-2)
    y_lib = ops.linear(x, gu, epilogue=1, policy="hipblaslt")
    torch.testing.assert_close(y.float(), y_lib.float(), atol=3e-2, rtol=3e-2)
    r = bf(torch.randn(M, F, device=DEV))
    w2 = bf(torch.randn(F, K, device=DEV) * 0.02)
    y2 = ops.linear(x, w2, epilogue=2, residual=r, policy="native", wp=ops.pack_weight(w2))
    torch.testing.assert_close(y2.float(), x.float() @ w2.float().t() + r.float(), atol=5e-2, rtol=3e-2)


@pytest.mark.parametrize("sk", ["on", "off"])
@pytest.mark.parametrize("M", [1, 16, 17, 48, 64])
@pytest.mark.parametrize("N,K", [(4096, 4096), (12288, 4096), (4096, 11008), (1024, 1024), (22016, 4096),
                                 (32000, 4096), (192, 8192)])
def test_gemm_stream_k(M, N, K, sk):
    """Stream-K decode GEMM (split groups, cross-workgroup slab fixup) vs fp32 reference;
    repeated launches must be bit-identical (counters re-zeroed, fixed reduction order)."""
    x = bf(torch.randn(M, K, device=DEV))
    w = bf(torch.randn(N, K, device=DEV) * 0.02)
    wp = ops.pack_weight(w)
    xp = ops.pack_act(x)
    ops.set_gemm_sk(sk)
    try:
        y1 = ops.linear(xp, None, wp=wp, a_rows=M)
        y2 = ops.linear(xp, None, wp=wp, a_rows=M)
        y3 = ops.linear(x, None, policy="native", wp=wp)
    finally:
        ops.set_gemm_sk("off")
    torch.cuda.synchronize()
    yr = x.float() @ w.float().t()
    torch.testing.assert_close(y1.float(), yr, atol=3e-2, rtol=2e-2)
    assert torch.equal(y1, y2)
    assert torch.equal(y1, y3)
    assert int(ops.gemm_workspace(DEV)[:4 * 4096].view(torch.int32).abs().sum()) == 0  # counters re-zeroed


@pytest.mark.parametrize("kern", ["lds22", "lds24", "lds42", "rw", "rwk", "rwki", "rwr", "pk+r", "lds24+r", "rw+r",
                                  "rwk+r", "rwki+r", "rwr+r"])
@pytest.mark.parametrize("M", [1, 16, 20, 40, 48, 64])
@pytest.mark.parametrize("N,K,epi", [(4096, 4096, 0), (12288, 4096, 2), (4096, 11008, 0), (22016, 4096, 1),
                                     (32000, 4096, 0), (1024, 1024, 1)])
def test_gemm_shared_a(kern, M, N, K, epi):
    """Shared-A (LDS-staged activation) and balanced-ring decode GEMMs, every epilogue, vs fp32;
    deterministic."""
    from src.models.weights import interleave_gate_up

    x = bf(torch.randn(M, K, device=DEV))
    w = bf(torch.randn(N, K, device=DEV) * 0.02)
    r = bf(torch.randn(M, N, device=DEV)) if epi == 2 else None
    wp = ops.pack_weight(w)
    xp = ops.pack_act(x)
    ops.set_gemm_sk(kern)
    try:
        applies = ops._kernel_for(M, N, K, epi) == kern
        y1 = ops.linear(xp, None, wp=wp, a_rows=M, epilogue=epi, residual=r, out_packed=epi == 1)
        y2 = ops.linear(xp, None, wp=wp, a_rows=M, epilogue=epi, residual=r, out_packed=epi == 1)
    finally:
        ops.set_gemm_sk("off")
    torch.cuda.synchronize()
    if epi == 1:  # packed output: padding rows are never written, compare the M real rows
        y1, y2 = ops.unpack_act(y1, M, N // 2), ops.unpack_act(y2, M, N // 2)
    assert torch.equal(y1, y2)
    yr = x.float() @ w.float().t()
    if epi == 1:  # rows interleaved [g16 u16 g16 u16 ...]
        gt = w.view(N // 32, 2, 16, K)
        g = x.float() @ gt[:, 0].reshape(-1, K).float().t()
        u = x.float() @ gt[:, 1].reshape(-1, K).float().t()
        yr = torch.nn.functional.silu(g) * u
    elif epi == 2:
        yr = yr + r.float()
    torch.testing.assert_close(y1.float(), yr, atol=4e-2, rtol=3e-2)
    base = ops._base(kern)
    if M == 64 and N in (22016, 32000) and base not in ("rwk", "rwki", "rwr", "pk"):
        assert applies  # the kernel itself ran (not the fallback)
    if base in ("rwk", "rwki") and N % 2048 == 0 and epi != 1:
        assert applies
    if base == "rwr" and N % 2048 == 0 and epi != 1 and (M + 15) // 16 in (2, 4):
        assert applies


@pytest.mark.parametrize("M", [5, 33, 64])
def test_gemm_stream_k_swiglu_packed_out(M):
    K, F = 4096, 11008
    from src.models.weights import interleave_gate_up

    x = bf(torch.randn(M, K, device=DEV))
    gate = bf(torch.randn(F, K, device=DEV) * 0.02)
    up = bf(torch.randn(F, K, device=DEV) * 0.02)
    gu = interleave_gate_up(gate, up)
    wp = ops.pack_weight(gu)
    ops.set_gemm_sk("on")
    try:
        yp = ops.linear(ops.pack_act(x), None, epilogue=1, wp=wp, a_rows=M, out_packed=True)
        y = ops.linear(x, None, epilogue=1, policy="native", wp=wp)
    finally:
        ops.set_gemm_sk("off")
    g, u = x.float() @ gate.float().t(), x.float() @ up.float().t()
    torch.testing.assert_close(y.float(), torch.nn.functional.silu(g) * u, atol=3e-2, rtol=3e-2)
    assert torch.equal(ops.unpack_act(yp, M, F), y)


def test_sampler_greedy_and_topk1():
    R, V = 6, 32000
    logits = bf(torch.randn(R, V, device=DEV) * 3)
    z = torch.zeros(R, dtype=torch.float32, device=DEV)
    args = dict(top_ps=torch.full((R,), 0.9, device=DEV), top_ks=torch.zeros(R, dtype=torch.int32, device=DEV),
                rep_pens=torch.ones(R, device=DEV), recent=torch.zeros(R, 50, dtype=torch.int32, device=DEV),
                recent_len=torch.zeros(R, dtype=torch.int32, device=DEV),
                seeds=torch.arange(R, dtype=torch.long, device=DEV))
    out = ops.sample(logits, z, **args)
    assert torch.equal(out, torch.argmax(logits.float(), -1))
    args["top_ks"] = torch.ones(R, dtype=torch.int32, device=DEV)
    out = ops.sample(logits, torch.ones(R, device=DEV), **args)
    assert torch.equal(out, torch.argmax(logits.float(), -1))


def test_sampler_repetition_penalty_blocks_repeats():
    V = 1000
    logits = torch.zeros(1, V, device=DEV)
    logits[0, 5] = 4.0
    logits[0, 6] = 3.9
    logits = bf(logits)
    hist = torch.zeros(1, 50, dtype=torch.int32, device=DEV)
    hist[0, :3] = 5
    kw = dict(top_ps=torch.ones(1, device=DEV), top_ks=torch.ones(1, dtype=torch.int32, device=DEV),
              rep_pens=torch.full((1,), 1.5, device=DEV), recent=hist,
              recent_len=torch.tensor([3], dtype=torch.int32, device=DEV),
              seeds=torch.tensor([1], device=DEV))
    out = ops.sample(logits, torch.ones(1, device=DEV), **kw)
    assert out.item() == 6  # 5 was penalised by 1.5**3 * 1.5**3
    assert ref.sample_row(logits[0].cpu(), 1.0, 1.0, 1, 1.5, [5, 5, 5]) == 6


def test_sampler_distribution_matches_reference():
    V = 64
    base = torch.randn(V) * 2
    logits = bf(base.to(DEV).unsqueeze(0).repeat(4096, 1))
    R = logits.shape[0]
    kw = dict(top_ps=torch.full((R,), 0.8, device=DEV), top_ks=torch.full((R,), 10, dtype=torch.int32, device=DEV),
              rep_pens=torch.ones(R, device=DEV), recent=torch.zeros(R, 50, dtype=torch.int32, device=DEV),
              recent_len=torch.zeros(R, dtype=torch.int32, device=DEV),
              seeds=torch.arange(R, dtype=torch.long, device=DEV) * 7 + 3)
    out = ops.sample(logits, torch.full((R,), 0.7, device=DEV), **kw).cpu()
    # expected distribution: reference semantics computed exactly
    p = torch.softmax(logits[0].float().cpu() / 0.7, -1)
    tv, ti = torch.topk(p, 10)
    q = torch.zeros_like(p).scatter(0, ti, tv)
    sp, si = torch.sort(q, descending=True)
    keep = torch.cumsum(sp, 0) <= 0.8
    keep[0] = True
    f = torch.zeros_like(p).scatter(0, si, sp * keep)
    f = f / f.sum()
    freq = torch.bincount(out, minlength=V).float() / R
    assert set(out.unique().tolist()) <= set(torch.nonzero(f).flatten().tolist())
    assert (freq - f).abs().max().item() < 0.04


@pytest.mark.parametrize("M", [1, 13, 16, 40, 64])
def test_packed_activation_paths(M):
    """Producers that emit the packed decode-GEMM layout agree with pack(row-major)."""
    H, K2 = 4096, 11008
    x = bf(torch.randn(M, H, device=DEV))
    assert torch.equal(ops.pack_act(x)[: ops.packed_numel(M, H)].view(-1)[: M * 0 + 1].cpu(),
                       ref.pack_act(x.cpu())[:1])
    ap = torch.zeros(ops.packed_numel(M, H), dtype=torch.bfloat16, device=DEV)
    ops.pack_act(x, out=ap)
    assert torch.equal(ref.unpack_act(ap.cpu(), M, H), x.cpu())
    w = bf(torch.rand(H, device=DEV) + 0.5)
    res = bf(torch.randn(M, H, device=DEV))
    r1, r2 = res.clone(), res.clone()
    yp = ops.rmsnorm(x, w, 1e-5, residual=r1, mode=1, packed=True)
    y = ops.rmsnorm(x, w, 1e-5, residual=r2, mode=1)
    assert torch.equal(ref.unpack_act(yp.cpu(), M, H), y.cpu())
    # GEMM on packed A == GEMM on row-major A
    wt = bf(torch.randn(12288, H, device=DEV) * 0.02)
    wp = ops.pack_weight(wt)
    g1 = ops.linear(y, None, wp=wp, policy="native")
    g2 = ops.linear(yp, None, wp=wp, a_rows=M)
    assert torch.equal(g1, g2)
    # SwiGLU epilogue emitting packed output feeds the down projection
    from src.models.weights import interleave_gate_up

    gu = interleave_gate_up(bf(torch.randn(K2, H, device=DEV) * 0.02), bf(torch.randn(K2, H, device=DEV) * 0.02))
    gup = ops.pack_weight(gu)
    a_row = ops.linear(yp, None, wp=gup, epilogue=1, a_rows=M)
    a_pk = ops.linear(yp, None, wp=gup, epilogue=1, a_rows=M, out_packed=True)
    assert torch.equal(ref.unpack_act(a_pk.cpu(), M, K2), a_row.cpu())
    wd = bf(torch.randn(H, K2, device=DEV) * 0.02)
    d1 = ops.linear(a_row, None, wp=ops.pack_weight(wd), policy="native")
    d2 = ops.linear(a_pk, None, wp=ops.pack_weight(wd), a_rows=M)
    assert torch.equal(d1, d2)


def test_paged_attention_packed_output():
    nh, nkv, D = 32, 32, 128
    q, kc, vc, bt, q_seq, q_ctx = _attn_case(nh, nkv, D, [100, 7, 600])
    for parts in [(64, 10), (1024, 1)]:
        o = ops.paged_attention(q, kc, vc, bt, q_seq, q_ctx, nh, nkv, 0.09, part_size=parts[0], num_parts=parts[1])
        op = ops.paged_attention(q, kc, vc, bt, q_seq, q_ctx, nh, nkv, 0.09, part_size=parts[0], num_parts=parts[1],
                                 packed=True)
        assert torch.equal(ref.unpack_act(op.cpu(), 3, nh * D), o.cpu())


@pytest.mark.parametrize("M", [1, 17, 64])
def test_fp8_quant_act_kernel_matches_reference(M):
    from src.ops import reference as ref

    K = 4096
    x = bf(torch.randn(M, K, device=DEV) * 3)
    xp = ops.pack_act(x)
    a8, s = ops.quant_act_fp8(xp, M, K)
    a8r, sr = ref.quant_act_fp8(xp.cpu(), M, K)
    torch.testing.assert_close(s[:M].cpu(), sr[:M], rtol=1e-6, atol=0)
    MT = (M + 15) // 16
    got = ref.dequant_act_fp8(a8.cpu(), sr, M, K)  # same scales: compare the fp8 codes
    want = ref.dequant_act_fp8(a8r, sr, M, K)
    # identical up to round-half ties of 1/scale vs *1/448 (1 fp8 ulp on a handful of elements)
    assert (got != want).float().mean() < 2e-2
    # <= 1 e4m3 ulp: relative 1/8 for normals, one subnormal step (2^-9 x the row scale) below
    torch.testing.assert_close(got, want, atol=float(sr[:M].max()) * 2.0 ** -9, rtol=0.13)
    assert a8.numel() >= MT * 16 * K


@pytest.mark.parametrize("kern", ["pk", "rw", "rwk"])
@pytest.mark.parametrize("M", [1, 30, 64])
@pytest.mark.parametrize("N,K,epi", [(1024, 1024, 0), (10240, 8192, 0), (8192, 28672, 0), (2048, 4096, 1),
                                     (4096, 11008, 2), (57344, 512, 1)])
def test_fp8_gemm_kernel_matches_reference(kern, M, N, K, epi):
    """Both fp8 GEMM forms vs the CPU reference; (57344, 512, 1) is the Llama-3-70B gate/up width
    (7 gate/up pairs per CU in the balanced ring form) at a short K."""
    from src.ops import reference as ref
    from src.models.weights import interleave_gate_up

    ops.set_fp8_kernel(kern)
    try:
        _fp8_gemm_case(M, N, K, epi, ref, interleave_gate_up)
    finally:
        ops.set_fp8_kernel("auto")


@pytest.mark.parametrize("kern", ["rw", "rwk", "rwki", "rw+r", "rwk+r", "rwki+r"])
@pytest.mark.parametrize("M", [1, 30, 64])
@pytest.mark.parametrize("N,K,epi", [(1024, 1024, 0), (10240, 8192, 0), (8192, 8192, 3), (8192, 28672, 3),
                                     (2048, 4096, 1), (57344, 512, 1), (4096, 1024, 0)])
def test_w8a16_gemm_matches_dequantized_reference(kern, M, N, K, epi, monkeypatch):
    """W8A16 decode GEMM (fp8 weights dequantized into the bf16 MFMA) vs x @ dequant(W)^T in fp32;
    epilogue 0 with and without the fused-norm row scale, packed SwiGLU (57344 = the Llama-3-70B
    gate/up width: 14 tiles per CU), and the residual-stream producer (residual, packed copy, row
    sums of squares) in both the ring and the split-K ring forms."""
    from src.models.weights import interleave_gate_up

    monkeypatch.setattr(ops, "_W8_MODE", kern)
    x = bf(torch.randn(M, K, device=DEV))
    if epi == 1:
        w = interleave_gate_up(torch.randn(N // 2, K, device=DEV) * 0.02, torch.randn(N // 2, K, device=DEV) * 0.02)
    else:
        w = torch.randn(N, K, device=DEV) * 0.02
    wq, ws = ops.pack_weight_fp8(w)
    w8 = ops.w8_from_fp8(wq)
    wdq = ops.unpack_weight_w8(w8, ws, torch.float32)
    wbf = wdq.to(torch.bfloat16).float()  # the kernel rounds the dequantized weight to bf16
    xp = ops.pack_act(x)
    exact = x.float() @ wbf.t()
    if epi == 0:
        y = ops.linear_w8(xp, w8, ws, M)
        torch.testing.assert_close(y.float(), exact, atol=5e-2, rtol=2e-2)
        assert float((y.float() - exact).norm() / exact.norm()) < 1e-2  # bf16 outputs: 2^-8 relative
        # fused-norm consumer: row scale rsqrt(ss / K + eps) from the fixed-point row statistics
        ss = ops.norm_stats_buffer(DEV)[0]
        ss.zero_()
        sq = (x.float() ** 2).sum(1)
        ss[0, :M] = torch.round(sq * 2.0 ** 20).long()
        y2 = ops.linear_w8(xp, w8, ws, M, ss_in=ss, eps=1e-5)
        want = exact * torch.rsqrt(sq / K + 1e-5)[:, None]
        torch.testing.assert_close(y2.float(), want, atol=5e-2, rtol=2e-2)
        assert float((y2.float() - want).norm() / want.norm()) < 1e-2  # bf16 outputs: 2^-8 relative
    elif epi == 1:
        yp = ops.linear_w8(xp, w8, ws, M, epilogue=1, out_packed=True)
        y = ops.unpack_act(yp, M, N // 2).float()
        g, u = exact.view(M, N // 32, 2, 16)[:, :, 0].reshape(M, N // 2), \
            exact.view(M, N // 32, 2, 16)[:, :, 1].reshape(M, N // 2)
        want = torch.nn.functional.silu(g) * u
        torch.testing.assert_close(y, want, atol=5e-2, rtol=2e-2)
        assert float((y - want).norm() / want.norm()) < 1e-2  # bf16 outputs: 2^-8 relative
    else:
        res = bf(torch.randn(M, N, device=DEV))
        r0 = res.clone()
        ap = torch.zeros(ops.packed_numel(M, N), dtype=torch.bfloat16, device=DEV)
        ss_out, ss_zero = ops.norm_stats_buffer(DEV, 2)
        ss_out.zero_()
        ops.linear_w8(xp, w8, ws, M, out=res, epilogue=3, residual=res, ap_out=ap, ss_out=ss_out, ss_zero=ss_zero)
        want = exact + r0.float()
        torch.testing.assert_close(res.float(), want, atol=6e-2, rtol=2e-2)  # two bf16 roundings of ~|8|
        assert torch.equal(ops.unpack_act(ap, M, N), res)
        got_ss = ss_out.view(-1, 64).sum(0)[:M].double() / 2.0 ** 20
        torch.testing.assert_close(got_ss, (res.double() ** 2).sum(1), rtol=1e-4, atol=1e-3)


def _fp8_gemm_case(M, N, K, epi, ref, interleave_gate_up):

    x = bf(torch.randn(M, K, device=DEV))
    if epi == 1:
        w = interleave_gate_up(torch.randn(N // 2, K, device=DEV) * 0.02, torch.randn(N // 2, K, device=DEV) * 0.02)
    else:
        w = torch.randn(N, K, device=DEV) * 0.02
    wq, ws = ops.pack_weight_fp8(w)
    a8, s = ops.quant_act_fp8(ops.pack_act(x), M, K)
    res = bf(torch.randn(M, N, device=DEV)) if epi == 2 else None
    y = ops.linear_fp8(a8, s, wq, ws, M, epilogue=epi, residual=res)
    yr = ref.linear_fp8(a8.cpu(), s.cpu(), wq.cpu(), ws.cpu(), M, epilogue=epi,
                        residual=None if res is None else res.cpu())
    torch.testing.assert_close(y.float().cpu(), yr.float(), atol=2e-2, rtol=2e-2)
    if epi == 1:
        yp = ops.linear_fp8(a8, s, wq, ws, M, epilogue=1, out_packed=True)
        assert torch.equal(ops.unpack_act(yp, M, N // 2), y)
    # vs the unquantized product: fp8 error budget
    if epi == 0:
        exact = x.float() @ w.float().t()
        assert float((y.float() - exact).norm() / exact.norm()) < 0.06


@pytest.mark.parametrize("k,tp", [(50, 0.92), (0, 0.92), (50, 1.0), (200, 0.92)])
def test_sampler_large_vocab_distribution(k, tp):
    """V = 32000 at the reference CLI defaults: fast top-k candidate path (k > 0; its candidate
    bound from the per-wave maxima for k <= 128, the exact radix select above) and the general
    radix path (k = 0) all sample the reference's filtered distribution."""
    V, R = 32000, 8192
    g = torch.Generator().manual_seed(11)
    base = torch.randn(V, generator=g) * 1.5
    base[:20] += 6  # a peaked head, like real LM logits
    logits = bf(base.to(DEV).unsqueeze(0).repeat(R, 1))
    kw = dict(top_ps=torch.full((R,), tp, device=DEV), top_ks=torch.full((R,), k, dtype=torch.int32, device=DEV),
              rep_pens=torch.ones(R, device=DEV), recent=torch.zeros(R, 50, dtype=torch.int32, device=DEV),
              recent_len=torch.zeros(R, dtype=torch.int32, device=DEV),
              seeds=torch.arange(R, dtype=torch.long, device=DEV) * 13 + 1)
    out = ops.sample(logits, torch.ones(R, device=DEV), **kw).cpu()
    p = torch.softmax(logits[0].float().cpu(), -1)
    q = p
    allowed = torch.ones(V, dtype=torch.bool)
    if 0 < k < V:
        tv, ti = torch.topk(p, k)
        q = torch.zeros_like(p).scatter(0, ti, tv)
        allowed = p >= tv[-1]  # bf16 logits tie: any id tied with the k-th value is a valid pick
    if 0 < tp < 1:
        sp, si = torch.sort(q, descending=True)
        cum = torch.cumsum(sp, 0)
        keep = cum <= tp
        keep[0] = True
        q = torch.zeros_like(p).scatter(0, si, sp * keep)
        allowed &= p >= sp[keep].min() * (1 - 1e-6)
    f = q / q.sum()
    freq = torch.bincount(out, minlength=V).float() / R
    assert set(out.unique().tolist()) <= set(torch.nonzero(allowed).flatten().tolist())
    assert (freq - f).abs().max().item() < 0.03


def test_sampler_history_update_and_degenerate_row():
    R, V = 3, 32000
    logits = torch.zeros(R, V, device=DEV)
    logits[1, 123] = 50.0
    logits = bf(logits)  # row 0 / 2: all-equal logits -> > 1024 top-k candidates (general path)
    recent = torch.zeros(R, 50, dtype=torch.int32, device=DEV)
    recent_len = torch.tensor([0, 50, 3], dtype=torch.int32, device=DEV)
    recent[1] = torch.arange(50, dtype=torch.int32, device=DEV) + 1000
    recent[2, :3] = torch.tensor([7, 8, 9], dtype=torch.int32, device=DEV)
    kw = dict(top_ps=torch.full((R,), 0.9, device=DEV), top_ks=torch.full((R,), 50, dtype=torch.int32, device=DEV),
              rep_pens=torch.ones(R, device=DEV), seeds=torch.arange(R, device=DEV))
    out = ops.sample(logits, torch.ones(R, device=DEV), recent=recent, recent_len=recent_len, update_history=True,
                     **kw)
    o = out.cpu().tolist()
    assert o[1] == 123 and 0 <= o[0] < V and 0 <= o[2] < V
    assert recent_len.cpu().tolist() == [1, 50, 4]
    r = recent.cpu()
    assert r[0, 0] == o[0]
    assert r[1, :49].tolist() == list(range(1001, 1050)) and r[1, 49] == 123
    assert r[2, :4].tolist() == [7, 8, 9, o[2]]
    # greedy rows update too
    out2 = ops.sample(logits, torch.zeros(R, device=DEV), recent=recent, recent_len=recent_len,
                      update_history=True, **kw)
    assert out2.cpu().tolist()[1] == 123 and recent_len.cpu().tolist() == [2, 50, 5]


@pytest.mark.parametrize("nh,nkv,D", [(32, 32, 128), (32, 8, 128), (64, 8, 128), (16, 4, 128), (12, 12, 64)])
@pytest.mark.parametrize("ctxs,multi", [([70, 9, 1, 33], True), ([1, 5, 300, 1000], False), ([4097], False)])
def test_attention_mfma_matches_reference(nh, nkv, D, ctxs, multi):
    """MFMA flash attention: causal prefill blocks (multi=True) and GQA/MHA decode."""
    q, kc, vc, bt, q_seq, q_ctx = _attn_case(nh, nkv, D, ctxs, multi_q=multi)
    ntoks = ctxs if multi else [1] * len(ctxs)
    qb = torch.from_numpy(ops.query_blocks(ntoks, nh // nkv)).to(DEV)
    scale = 1 / math.sqrt(D)
    out = ops.attention_mfma(q, kc, vc, bt, q_seq, q_ctx, qb, nh, nkv, scale)
    o_ref = ref.paged_attention(q.float(), kc.float(), vc.float(), bt, q_seq, q_ctx, nh, nkv, scale)
    torch.testing.assert_close(out.float(), o_ref.float(), atol=2e-2, rtol=2e-2)
    # split-K partitions and the packed output layout
    outp = ops.attention_mfma(q, kc, vc, bt, q_seq, q_ctx, qb, nh, nkv, scale, part_size=128,
                              num_parts=math.ceil(max(ctxs) / 128), packed=True)
    torch.testing.assert_close(ops.unpack_act(outp, q.shape[0], nh * D).float(), o_ref.float(), atol=2e-2,
                               rtol=2e-2)


@pytest.mark.parametrize("nh,nkv,D", [(32, 32, 128), (32, 8, 128), (12, 12, 64), (64, 8, 128)])
@pytest.mark.parametrize("ntoks,prefix", [([70, 9, 1, 33, 130], [0, 0, 0, 0, 0]), ([300, 17], [64, 5]),
                                          ([1000], [0]), ([48, 64], [1, 200])])
@pytest.mark.parametrize("parts", [None, (128, 3)])
def test_attention_mfma_grouped_prefill(nh, nkv, D, ntoks, prefix, parts):
    """Grouped MFMA prefill (up to 4 query blocks of a sequence per workgroup sharing each K/V
    step) vs the fp32 reference: ragged prompts, chunked prefill over an existing prefix
    (ctx = prefix + i + 1), split-K partitions, packed output."""
    ctxs = [p + n for p, n in zip(prefix, ntoks)]
    q, kc, vc, bt, _, _ = _attn_case(nh, nkv, D, ctxs)
    q_seq = torch.cat([torch.full((n,), i, dtype=torch.int32) for i, n in enumerate(ntoks)]).to(DEV)
    q_ctx = torch.cat([torch.arange(p + 1, p + n + 1, dtype=torch.int32) for p, n in zip(prefix, ntoks)]).to(DEV)
    T = q_seq.numel()
    q = bf(torch.randn(T, (nh + 2 * nkv) * D, device=DEV))
    qb = torch.from_numpy(ops.query_blocks(ntoks, nh // nkv)).to(DEV)
    sb = torch.from_numpy(ops.query_superblocks(ntoks, nh // nkv)).to(DEV)
    assert int(sb[1].sum()) == qb.shape[1] and int(sb[1].max()) <= 8
    scale = 1 / math.sqrt(D)
    kw = {} if parts is None else dict(part_size=parts[0], num_parts=math.ceil(max(ctxs) / parts[0]))
    out = ops.attention_mfma(q, kc, vc, bt, q_seq, q_ctx, qb, nh, nkv, scale, superblocks=sb, **kw)
    o_ref = ref.paged_attention(q.float(), kc.float(), vc.float(), bt, q_seq, q_ctx, nh, nkv, scale)
    torch.testing.assert_close(out.float(), o_ref.float(), atol=2e-2, rtol=2e-2)
    outp = ops.attention_mfma(q, kc, vc, bt, q_seq, q_ctx, qb, nh, nkv, scale, superblocks=sb, packed=True, **kw)
    torch.testing.assert_close(ops.unpack_act(outp, T, nh * D).float(), o_ref.float(), atol=2e-2, rtol=2e-2)


@pytest.mark.parametrize("nh,nkv", [(32, 32), (32, 8), (64, 8), (16, 8), (8, 4)])
@pytest.mark.parametrize("ntoks,prefix", [([70, 9, 1, 33, 130], [0, 0, 0, 0, 0]), ([300, 17], [64, 5]),
                                          ([1000], [0]), ([48, 64], [1, 200]), ([129, 256], [0, 63])])
@pytest.mark.parametrize("waves,parts,pair", [(4, None, False), (8, None, False), (4, 3, False), (4, None, True),
                                             (8, None, True)])
def test_attention_fa_prefill(nh, nkv, ntoks, prefix, waves, parts, pair):
    """FA2 prefill kernel (32x32x16 MFMA, transposed LDS reads of V) vs the fp32 reference:
    ragged prompts, chunked prefill over an existing prefix (ctx = prefix + i + 1), 4- and
    8-wave workgroups, context split over parts, causal block pairing (a workgroup runs a long
    block and its short mirror; odd block counts leave one unpaired).  Cache slots past every
    context hold NaN: they must never reach the output."""
    D = 128
    ctxs = [p + n for p, n in zip(prefix, ntoks)]
    q, kc, vc, bt, _, _ = _attn_case(nh, nkv, D, ctxs)
    ps = kc.shape[2]
    for i, c in enumerate(ctxs):  # poison the unused tail of every sequence's last page
        pg = int(bt[i, (c - 1) // ps])
        kc[pg, :, (c - 1) % ps + 1:] = float("nan")
        vc[pg, :, (c - 1) % ps + 1:] = float("nan")
    q_seq = torch.cat([torch.full((n,), i, dtype=torch.int32) for i, n in enumerate(ntoks)]).to(DEV)
    q_ctx = torch.cat([torch.arange(p + 1, p + n + 1, dtype=torch.int32) for p, n in zip(prefix, ntoks)]).to(DEV)
    T = q_seq.numel()
    q = bf(torch.randn(T, (nh + 2 * nkv) * D, device=DEV))
    fb = torch.from_numpy(ops.fa_blocks(ntoks, nh // nkv, waves)).to(DEV)
    assert int(fb[1].sum()) == T
    scale = 1 / math.sqrt(D)
    out = ops.attention_fa(q, kc, vc, bt, q_seq, q_ctx, fb, nh, nkv, scale, waves=waves, num_parts=parts, pair=pair)
    kr, vr = kc.clone(), vc.clone()
    kr[kr.isnan()] = 0
    vr[vr.isnan()] = 0
    o_ref = ref.paged_attention(q.float(), kr.float(), vr.float(), bt, q_seq, q_ctx, nh, nkv, scale)
    assert torch.isfinite(out.float()).all()
    torch.testing.assert_close(out.float(), o_ref.float(), atol=2e-2, rtol=2e-2)


def test_fa_blocks():
    assert ops.fa_blocks([5, 1, 300], 1, 4).tolist() == [[0, 5, 6, 134, 262], [5, 1, 128, 128, 44]]
    assert ops.fa_blocks([40], 4, 4).tolist() == [[0, 32], [32, 8]]
    assert ops.fa_blocks([40], 8, 8).tolist() == [[0, 32], [32, 8]]
    fb = ops.fa_blocks([], 4, 4)  # an empty step: no blocks, still [2, 0] int32
    assert fb.shape == (2, 0) and fb.dtype == np.int32


def test_query_superblocks():
    assert ops.query_superblocks([5, 1, 70], 1).tolist() == [[0, 1, 2], [1, 1, 5]]
    assert ops.query_superblocks([5, 1, 70], 1, group=4).tolist() == [[0, 1, 2, 6], [1, 1, 4, 1]]
    assert ops.query_superblocks([16], 4).tolist() == [[0], [4]]
    assert ops.query_superblocks([40], 4).tolist() == [[0, 8], [8, 2]]


def test_query_blocks():
    qb = ops.query_blocks([5, 1, 17], 1)
    assert qb.tolist() == [[0, 5, 6, 22], [5, 1, 16, 1]]
    qb = ops.query_blocks([5, 1], 8)  # 2 tokens x 8 heads per block
    assert qb.tolist() == [[0, 2, 4, 5], [2, 2, 1, 1]]
    qb = ops.query_blocks([], 8)  # an empty step: no blocks, still [2, 0] int32
    assert qb.shape == (2, 0) and qb.dtype == np.int32


@pytest.mark.parametrize("nh,nkv,D", [(32, 32, 128), (32, 8, 128), (12, 12, 64)])
@pytest.mark.parametrize("parts", [None, (64, 8)])
@pytest.mark.parametrize("packed", [False, True])
def test_paged_attention_rope_fused_matches_two_kernels(nh, nkv, D, parts, packed):
    """Decode attention with RoPE + KV write folded in == rope_kv_write then paged_attention
    (and the fp32 reference); the cache receives the same rotated k / copied v; a padded row
    (ctx 0, slot -1) writes nothing and outputs 0."""
    ctxs = [1, 5, 64, 200, 0]
    ps = 64
    q, kc, vc, bt, q_seq, q_ctx = _attn_case(nh, nkv, D, [max(c, 1) for c in ctxs], ps=ps)
    q_ctx[-1] = 0
    pos = (q_ctx.long() - 1).clamp(min=0)
    slots = torch.stack([bt[i, int(p) // ps].long() * ps + int(p) % ps for i, p in enumerate(pos.tolist())])
    slots[-1] = -1
    cos, sin = ops.rope_cos_sin(D, 2048, 10000.0, DEV)
    scale = 1 / math.sqrt(D)
    kw = dict(part_size=parts[0], num_parts=parts[1]) if parts else dict(max_ctx=max(ctxs))
    k2, v2, q2 = kc.clone(), vc.clone(), q.clone()
    ops.rope_kv_write(q2, pos, cos, sin, k2, v2, slots, nh, nkv)
    o2 = ops.paged_attention(q2, k2, v2, bt, q_seq, q_ctx, nh, nkv, scale, packed=packed, **kw)
    q_in = q.clone()
    o1 = ops.paged_attention_rope(q, kc, vc, bt, q_seq, q_ctx, pos, cos, sin, slots, nh, nkv, scale,
                                  packed=packed, **kw)
    assert torch.equal(q, q_in), "fused op must not modify qkv"
    torch.testing.assert_close(kc.float(), k2.float(), atol=1e-2, rtol=1e-2)
    assert torch.equal(vc, v2)
    T = q.shape[0]
    if packed:
        o1, o2 = ref.unpack_act(o1, T, nh * D), ref.unpack_act(o2, T, nh * D)
    torch.testing.assert_close(o1.float(), o2.float(), atol=2e-2, rtol=2e-2)
    if not packed:
        o_ref = ref.paged_attention(q2.float(), k2.float(), v2.float(), bt, q_seq, q_ctx, nh, nkv, scale)
        torch.testing.assert_close(o1.float(), o_ref.float(), atol=2e-2, rtol=2e-2)
        assert torch.count_nonzero(o1[-1]) == 0


def test_autotune_weight_larger_than_pool(monkeypatch):
    """A weight bigger than the rotation pool (Llama-3-70B's 128K-vocab lm_head vs the 1 GiB
    pool) is timed on one dedicated copy instead of failing to view the pool."""
    monkeypatch.setattr(ops, "_TUNE_POOL_BYTES", 1 << 20)
    monkeypatch.setenv("MPAMD_GEMM_AUTOTUNE", "1")  # (the suite runs from the committed table)
    N, K = 4096 + 16 * 7, 4096
    key = (64, N, K, 0)
    ops._SK_CHOICE.pop(key, None)
    table = ops.autotune_gemm([(N, K, 0)], DEV, ms=(64,), iters=2, rounds=1)
    assert ops._base(ops._SK_CHOICE.get(key)) in (set(ops._KERNEL_FLAGS) | {"pk"}), table
    ops._SK_CHOICE.pop(key, None)


@pytest.mark.parametrize("nh,nkv,D", [(32, 8, 128), (64, 8, 128), (16, 4, 128), (8, 2, 64), (32, 32, 128)])
@pytest.mark.parametrize("parts", [None, (128, 4)])
@pytest.mark.parametrize("packed", [False, True])
def test_attention_mfma_rope_fused_matches_two_kernels(nh, nkv, D, parts, packed):
    """GQA decode on the MFMA kernel with RoPE + KV write folded in == rope_kv_write then
    attention_mfma; same cache contents; a padded row (ctx 0, slot -1) writes nothing."""
    ctxs = [1, 5, 64, 200, 0, 33]
    ps = 64
    q, kc, vc, bt, q_seq, q_ctx = _attn_case(nh, nkv, D, [max(c, 1) for c in ctxs], ps=ps)
    q_ctx[4] = 0
    pos = (q_ctx.long() - 1).clamp(min=0)
    slots = torch.stack([bt[i, int(p) // ps].long() * ps + int(p) % ps for i, p in enumerate(pos.tolist())])
    slots[4] = -1
    qb = torch.from_numpy(ops.query_blocks([1] * len(ctxs), nh // nkv)).to(DEV)
    cos, sin = ops.rope_cos_sin(D, 2048, 10000.0, DEV)
    scale = 1 / math.sqrt(D)
    kw = dict(part_size=parts[0], num_parts=parts[1]) if parts else dict(max_ctx=max(ctxs))
    k2, v2, q2 = kc.clone(), vc.clone(), q.clone()
    ops.rope_kv_write(q2, pos, cos, sin, k2, v2, slots, nh, nkv)
    o2 = ops.attention_mfma(q2, k2, v2, bt, q_seq, q_ctx, qb, nh, nkv, scale, packed=packed, **kw)
    q_in = q.clone()
    o1 = ops.attention_mfma_rope(q, kc, vc, bt, q_seq, q_ctx, qb, pos, cos, sin, slots, nh, nkv, scale,
                                 packed=packed, **kw)
    assert torch.equal(q, q_in), "fused op must not modify qkv"
    torch.testing.assert_close(kc.float(), k2.float(), atol=1e-2, rtol=1e-2)
    assert torch.equal(vc, v2)
    T = q.shape[0]
    if packed:
        o1, o2 = ref.unpack_act(o1, T, nh * D), ref.unpack_act(o2, T, nh * D)
    torch.testing.assert_close(o1.float(), o2.float(), atol=2e-2, rtol=2e-2)
    o_ref = ref.paged_attention(q2.float(), k2.float(), v2.float(), bt, q_seq, q_ctx, nh, nkv, scale)
    torch.testing.assert_close(o1.float(), o_ref.float(), atol=2e-2, rtol=2e-2)


@pytest.mark.parametrize("M", [65, 96, 113, 128])
@pytest.mark.parametrize("N,K,epi", [(4096, 4096, 0), (12288, 4096, 0), (4096, 11008, 0), (22016, 4096, 1),
                                     (1536, 512, 0), (2048, 512, 1)])
def test_gemm_wide_rows_65_to_128(M, N, K, epi):
    """65..128 decode rows (96 / 128 sessions) stay on the hand-written balanced ring kernel:
    plain and packed-SwiGLU epilogues vs fp32 x @ w.T; deterministic."""
    from src.models.weights import interleave_gate_up

    assert ops.native_gemm_ok(M, N, K, epi, epi == 1)
    x = bf(torch.randn(M, K, device=DEV))
    if epi == 1:
        w = bf(interleave_gate_up(torch.randn(N // 2, K, device=DEV) * 0.02, torch.randn(N // 2, K, device=DEV) * 0.02))
    else:
        w = bf(torch.randn(N, K, device=DEV) * 0.02)
    wp = ops.pack_weight(w)
    xp = ops.pack_act(x)
    y1 = ops.linear(xp, None, wp=wp, a_rows=M, epilogue=epi, out_packed=epi == 1)
    y2 = ops.linear(xp, None, wp=wp, a_rows=M, epilogue=epi, out_packed=epi == 1)
    torch.cuda.synchronize()
    if epi == 1:
        y1, y2 = ops.unpack_act(y1, M, N // 2), ops.unpack_act(y2, M, N // 2)
    assert torch.equal(y1, y2)
    yr = x.float() @ w.float().t()
    if epi == 1:
        gt = w.view(N // 32, 2, 16, K)
        g = x.float() @ gt[:, 0].reshape(-1, K).float().t()
        u = x.float() @ gt[:, 1].reshape(-1, K).float().t()
        yr = torch.nn.functional.silu(g) * u
    torch.testing.assert_close(y1.float(), yr, atol=4e-2, rtol=3e-2)


def test_executor_wide_decode_batch_packed_path_matches_hipblaslt():
    """A 80-session decode step takes the packed path (ring kernel at MT = 5) and matches the
    row-major hipBLASLt path of the same executor weights."""
    from src.models.config import resolve_model
    from src.models.weights import random_stage_weights
    from src.runtime.executor import StageExecutor

    cfg = resolve_model("small-llama")
    w = random_stage_weights(cfg, 0, cfg.num_hidden_layers, has_embed=True, has_head=True, device=DEV, seed=9)
    n = 80
    gen = torch.Generator().manual_seed(1)
    prompts = [torch.randint(0, cfg.vocab_size, (3 + i % 5,), generator=gen) for i in range(n)]
    outs = []
    for policy in ("auto", "hipblaslt"):
        ops.set_gemm_policy(policy)
        try:
            ex = StageExecutor(cfg, w, DEV, kv_cache_bytes=512 << 20, max_sessions=96, max_seq_len=64, use_graphs=False)
            if policy == "auto":
                assert ex._packed_ok(n)
            seqs = [(f"s{i}", len(p)) for i, p in enumerate(prompts)]
            ex.forward(seqs, torch.cat(prompts).to(DEV), reset=[True] * n)
            tok = torch.arange(n, device=DEV) % cfg.vocab_size
            outs.append(ex.forward([(s, 1) for s, _ in seqs], tok).float())
        finally:
            ops.set_gemm_policy("auto")
    torch.testing.assert_close(outs[0], outs[1], atol=0.08, rtol=0.05)


@pytest.mark.gpu
@pytest.mark.parametrize("M,N,K", [(256, 12288, 4096), (256, 4096, 11008), (2048, 22016, 4096)])
def test_tuned_library_gemm_table_loads_and_matches_fp32(M, N, K):
    """The shipped TunableOp table (ops/tuned/gemm_gfx950.csv) loads on this ROCm build and
    the solutions it picks for the row-major shapes compute x @ w^T (fp32 reference)."""
    assert ops.use_tuned_gemms()
    g = torch.Generator(device=DEV).manual_seed(M + N)
    x = (torch.randn(M, K, device=DEV, generator=g) * 0.5).to(torch.bfloat16)
    w = (torch.randn(N, K, device=DEV, generator=g) * 0.02).to(torch.bfloat16)
    out = torch.empty(M, N, dtype=torch.bfloat16, device=DEV)
    y = ops.linear(x, w, out=out, policy="hipblaslt")
    torch.testing.assert_close(y.float(), x.float() @ w.float().t(), atol=2e-2, rtol=2e-2)


@pytest.mark.parametrize("M", [129, 192, 256])
@pytest.mark.parametrize("N,K,epi", [(4096, 4096, 0), (12288, 4096, 0), (22016, 4096, 1), (4096, 11008, 2)])
def test_linear_above_128_rows_matches_fp32(M, N, K, epi):
    """Decode steps of 129..256 rows (the 256-session bench): the projections run on hipBLASLt
    (shipped TunableOp solutions) with the framework's SwiGLU / residual epilogue kernels; vs
    fp32 x @ w.T (and silu(g) * u / + residual)."""
    ops.use_tuned_gemms()
    x = bf(torch.randn(M, K, device=DEV))
    w = bf(torch.randn(N, K, device=DEV) * 0.02)
    r = bf(torch.randn(M, N, device=DEV)) if epi == 2 else None
    wp = ops.pack_weight(w)  # present, as on the executor path: the dispatcher must still pick hipBLASLt
    y = ops.linear(x, w, epilogue=epi, residual=r, wp=wp)
    yr = x.float() @ w.float().t()
    if epi == 1:
        gt = w.view(N // 32, 2, 16, K)
        g = x.float() @ gt[:, 0].reshape(-1, K).float().t()
        u = x.float() @ gt[:, 1].reshape(-1, K).float().t()
        yr = torch.nn.functional.silu(g) * u
    elif epi == 2:
        yr = yr + r.float()
    assert y.shape == yr.shape
    torch.testing.assert_close(y.float(), yr, atol=4e-2, rtol=3e-2)


@pytest.mark.parametrize("k,tp", [(50, 0.92), (50, 1.0), (64, 0.5)])
def test_sampler_split_wide_vocab_distribution(k, tp):
    """V = 128256 (Llama-3): the split sampler (chunk top-k workgroups + a one-wave merge) samples
    the reference's top-k / top-p filtered distribution."""
    V, R = 128256, 2048
    g = torch.Generator().manual_seed(5)
    base = torch.randn(V, generator=g) * 1.5
    base[:20] += 6
    base[V - 7] += 7  # a head token in the last (partial) chunk
    logits = bf(base.to(DEV).unsqueeze(0).repeat(R, 1))
    kw = dict(top_ps=torch.full((R,), tp, device=DEV), top_ks=torch.full((R,), k, dtype=torch.int32, device=DEV),
              rep_pens=torch.ones(R, device=DEV), recent=torch.zeros(R, 50, dtype=torch.int32, device=DEV),
              recent_len=torch.zeros(R, dtype=torch.int32, device=DEV),
              seeds=torch.arange(R, dtype=torch.long, device=DEV) * 7 + 3)
    out = ops.sample(logits, torch.ones(R, device=DEV), **kw).cpu()
    p = torch.softmax(logits[0].float().cpu(), -1)
    tv, ti = torch.topk(p, k)
    q = torch.zeros_like(p).scatter(0, ti, tv)
    allowed = p >= tv[-1]
    if 0 < tp < 1:
        sp, si = torch.sort(q, descending=True)
        keep = torch.cumsum(sp, 0) <= tp
        keep[0] = True
        q = torch.zeros_like(p).scatter(0, si, sp * keep)
        allowed &= p >= sp[keep].min() * (1 - 1e-6)
    f = q / q.sum()
    freq = torch.bincount(out, minlength=V).float() / R
    assert set(out.unique().tolist()) <= set(torch.nonzero(allowed).flatten().tolist())
    assert (freq - f).abs().max().item() < 0.04


def test_sampler_split_mixed_rows_and_history():
    """Wide vocabulary, one launch with split rows (top-k), greedy rows (raw argmax, no penalty),
    rows the split hands to the single-workgroup kernel (k = 0, k > 64), repetition penalty, and
    the in-place history update on every row."""
    V, R = 128256, 6
    logits = torch.randn(R, V, device=DEV) * 0.5
    logits[:, 100_000] = 30.0  # the head token, in chunk 12
    logits[4, 5] = 29.0
    logits = bf(logits)
    temps = torch.tensor([1.0, 0.0, 1.0, 1.0, 1.0, 0.0], device=DEV)
    top_ks = torch.tensor([50, 50, 0, 100, 50, 10], dtype=torch.int32, device=DEV)
    rep = torch.tensor([1.0, 1.0, 1.0, 1.0, 1e4, 1e4], device=DEV)
    recent = torch.zeros(R, 50, dtype=torch.int32, device=DEV)
    recent[4, 0] = 100_000  # row 4: the head token is penalised away -> token 5 wins
    recent[5, 0] = 100_000  # row 5 is greedy: raw argmax, the penalty does not apply
    recent_len = torch.tensor([0, 0, 0, 0, 1, 1], dtype=torch.int32, device=DEV)
    out = ops.sample(logits, temps, torch.full((R,), 0.9, device=DEV), top_ks, rep, recent, recent_len,
                     torch.arange(R, device=DEV), update_history=True).cpu().tolist()
    assert out == [100_000, 100_000, 100_000, 100_000, 5, 100_000]
    assert recent_len.cpu().tolist() == [1, 1, 1, 1, 2, 2]
    r = recent.cpu()
    assert [int(r[i, 0]) for i in range(4)] == out[:4] and int(r[4, 1]) == 5 and int(r[5, 1]) == 100_000
