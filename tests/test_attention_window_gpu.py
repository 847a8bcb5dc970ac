"""Sliding-window attention on the GPU: the window probes (tests/attn_window_probe.py) through the
decode kernels, the unwindowed path bit for bit, random inputs against the reference, the launches
that refuse a window, and stage runs past the window against the windowed fp32 oracle.

Probes: every cache position below a row's ``lo = max(0, ctx - W)`` is NaN and the block-table
entries of the pages wholly below it name an all-NaN page, so a kernel that reads one key (or one
page id) too many returns a non-finite row; the keys probed sit at ``lo``, ``lo + 1``, ``ctx - 1``
and on both sides of every slice boundary as the kernel places it.  W in 1 / 33 / 64 / 100, contexts
1, W - 1, W, W + 1, W + 31, W + 32, W + 33, W + 64, 2 W + 65, W + 1000 in ONE launch: ``lo`` at 0, 1
and each side of a 32-token step and of a page.  The comparator allows 2^-6, derived in attn_probe.py.

Largest |out - closed form| measured on an MI355X over all window probes, for each of the eight kernels
(``pytest -s`` prints them as WINDOW_PROBE_DEV lines): 0.003795, the bf16 rounding of the output alone."""
import dataclasses
import functools
import math

import pytest
import torch

from src import ops
from src.models.config import resolve_model
from src.models.reference_model import reference_forward
from src.models.weights import random_stage_weights
from src.ops import reference as ref
from src.runtime.executor import StageExecutor
from tests import attn_probe as ap
from tests import attn_window_probe as wp

pytestmark = pytest.mark.gpu
DEV = "cuda"

FD_SHAPES = [(8, 2, 128), (12, 12, 64), (8, 2, 64)]
MFMA_SHAPES = [(32, 8, 128), (16, 4, 128), (16, 4, 64)]

_SEEN = {}


@pytest.fixture(scope="module", autouse=True)
def _native():
    assert ops.load_library(), "HIP kernel library must load on the GPU box"
    yield
    for k, v in sorted(_SEEN.items()):
        print(f"\nWINDOW_PROBE_DEV {k} {v:.6f}", end="")


def _note(kernel, dev):
    _SEEN[kernel] = max(_SEEN.get(kernel, 0.0), dev)


@functools.lru_cache(maxsize=None)
def _case(nh, nkv, D, W, mfma):
    return wp.window_case(nh, nkv, D, W, mfma=mfma)


@functools.lru_cache(maxsize=None)
def _rope(nh, nkv, D, W, mfma, quarter):
    return wp.window_rope_case(nh, nkv, D, W, mfma=mfma, quarter=quarter)


def _caches(case, a, f8):
    """Fresh caches of a launch (a RoPE launch writes them)."""
    if not f8:
        return a["k_cache"], a["v_cache"]
    return case.f8(DEV)


def _args(a):
    return a["block_tables"], a["q_seq"], a["q_ctx"]


def _qblocks(case):
    return torch.from_numpy(ops.query_blocks([1] * case.T, case.nh // case.nkv)).to(DEV)


# ------------------------------------------------------------------------------------ probes
@pytest.mark.parametrize("nh,nkv,D", FD_SHAPES)
@pytest.mark.parametrize("W", wp.WINDOWS)
@pytest.mark.parametrize("f8", [False, True])
def test_flash_decoding_window_probes(nh, nkv, D, W, f8, monkeypatch):
    case = _case(nh, nkv, D, W, False)
    a = case.to(DEV)
    kc, vc = _caches(case, a, f8)
    assert wp.default_part_size(case, W, False, False) in wp.FD_PARTS
    what = f"paged_attention{'_f8' if f8 else ''}"
    for inlaunch in (False, True):
        monkeypatch.setattr(ops, "ATTN_INLAUNCH_REDUCE", inlaunch)
        for ps, np_ in [(None, None)] + wp.window_partitions(case, W, False):
            kw = dict(part_size=ps, num_parts=np_) if ps else {}
            out = ops.paged_attention(a["q"], kc, vc, *_args(a), nh, nkv, case.scale, window=W, **kw)
            _note(what, ap.compare(out, case, f"{what} W={W} part {ps} x {np_} inlaunch={inlaunch}"))
    assert int(ops.attention_counters(DEV).abs().sum()) == 0


@pytest.mark.parametrize("nh,nkv,D", FD_SHAPES)
@pytest.mark.parametrize("W", wp.WINDOWS)
@pytest.mark.parametrize("f8", [False, True])
def test_paged_attention_rope_window_probes(nh, nkv, D, W, f8):
    what = f"paged_attention_rope{'_f8' if f8 else ''}"
    for quarter in (False, True):
        case = _rope(nh, nkv, D, W, False, quarter)
        for ps, np_ in [(None, None)] + wp.window_partitions(case, W, False):
            a = case.to(DEV)
            kc, vc = _caches(case, a, f8)
            kw = dict(part_size=ps, num_parts=np_) if ps else {}
            out = ops.paged_attention_rope(a["q"], kc, vc, *_args(a), a["positions"], a["cos"], a["sin"], a["slots"],
                                           nh, nkv, case.scale, window=W, **kw)
            _note(what, ap.compare(out, case, f"{what} W={W} part {ps} x {np_} quarter={quarter}"))
            assert torch.equal(a["q"].cpu(), case.q), "the fused op must not modify qkv"
            wp.check_cache_after(case, kc, vc, f8)  # only the new token's slot is written


@pytest.mark.parametrize("nh,nkv,D", MFMA_SHAPES)
@pytest.mark.parametrize("W", wp.WINDOWS)
@pytest.mark.parametrize("f8", [False, True])
def test_attention_mfma_window_probes(nh, nkv, D, W, f8):
    case = _case(nh, nkv, D, W, True)
    a = case.to(DEV)
    kc, vc = _caches(case, a, f8)
    qb = _qblocks(case)
    op = ops.attention_mfma_f8 if f8 else ops.attention_mfma
    assert wp.default_part_size(case, W, True, False) in wp.MFMA_PARTS
    what = f"attention_mfma{'_f8' if f8 else ''}"
    for ps, np_ in [(None, None)] + wp.window_partitions(case, W, True):
        kw = dict(part_size=ps, num_parts=np_) if ps else {}
        out = op(a["q"], kc, vc, *_args(a), qb, nh, nkv, case.scale, window=W, **kw)
        _note(what, ap.compare(out, case, f"{what} W={W} part {ps} x {np_}"))


@pytest.mark.parametrize("nh,nkv,D", MFMA_SHAPES)
@pytest.mark.parametrize("W", wp.WINDOWS)
@pytest.mark.parametrize("f8", [False, True])
def test_attention_mfma_rope_window_probes(nh, nkv, D, W, f8):
    op = ops.attention_mfma_rope_f8 if f8 else ops.attention_mfma_rope
    what = f"attention_mfma_rope{'_f8' if f8 else ''}"
    for quarter in (False, True):
        case = _rope(nh, nkv, D, W, True, quarter)
        assert wp.default_part_size(case, W, True, True) in wp.MFMA_PARTS
        qb = _qblocks(case)
        for ps, np_ in [(None, None)] + wp.window_partitions(case, W, True):
            a = case.to(DEV)
            kc, vc = _caches(case, a, f8)
            kw = dict(part_size=ps, num_parts=np_) if ps else {}
            out = op(a["q"], kc, vc, *_args(a), qb, a["positions"], a["cos"], a["sin"], a["slots"], nh, nkv,
                     case.scale, window=W, **kw)
            _note(what, ap.compare(out, case, f"{what} W={W} part {ps} x {np_} quarter={quarter}"))
            assert torch.equal(a["q"].cpu(), case.q), "the fused op must not modify qkv"
            wp.check_cache_after(case, kc, vc, f8)


def test_explicit_slices_must_cover_the_streamed_span():
    case = _case(8, 2, 64, 100, False)
    a = case.to(DEV)
    with pytest.raises(ValueError, match="cover"):
        ops.paged_attention(a["q"], a["k_cache"], a["v_cache"], *_args(a), 8, 2, case.scale, window=100, part_size=64,
                            num_parts=1, max_ctx=int(case.q_ctx.max()))
    with pytest.raises(ValueError, match="window"):
        ops.paged_attention(a["q"], a["k_cache"], a["v_cache"], *_args(a), 8, 2, case.scale, window=-1)
    ws = ops.attention_workspace(case.T, 8, 64, 1, DEV)
    out = torch.empty(case.T, 8 * 64, dtype=torch.bfloat16, device=DEV)
    with pytest.raises(RuntimeError, match="window"):  # the shared host check, below the Python layer
        torch.ops.mpamd.paged_attention(a["q"], a["k_cache"], a["v_cache"], *_args(a), out, ws, 8, 2, case.scale, 64, 1,
                                        0, None, -1)


# ------------------------------------------------------------------------------------ unwindowed path
@pytest.mark.parametrize("f8", [False, True])
def test_window_at_or_above_the_context_is_the_unwindowed_launch(f8):
    """ctx <= W: the same slices, the same arithmetic - ``torch.equal`` to window=0 for every kernel."""
    ctxs = (1, 63, 64, 65, 129, 257)
    mc = dict(max_ctx=max(ctxs))  # (explicit slices of a windowed launch are checked against it)
    for W in (257, 1000):
        for nh, nkv, D in ((8, 2, 128), (12, 12, 64)):
            case = ap.decode_case(nh, nkv, D, ctxs=ctxs, rows=2)
            a = case.to(DEV)
            kc, vc = _caches(case, a, f8)
            for kw in ({}, dict(part_size=64, num_parts=5), dict(part_size=256, num_parts=2)):
                o0 = ops.paged_attention(a["q"], kc, vc, *_args(a), nh, nkv, case.scale, **mc, **kw)
                o1 = ops.paged_attention(a["q"], kc, vc, *_args(a), nh, nkv, case.scale, window=W, **mc, **kw)
                assert torch.equal(o0, o1), (W, nh, kw)
            rc = ap.rope_case(nh, nkv, D, ctxs=ctxs)
            outs = []
            for w_ in (0, W):
                ra = rc.to(DEV)
                rk, rv = _caches(rc, ra, f8)
                outs.append((ops.paged_attention_rope(ra["q"], rk, rv, *_args(ra), ra["positions"], ra["cos"], ra["sin"],
                                                      ra["slots"], nh, nkv, rc.scale, window=w_, part_size=64,
                                                      num_parts=5, **mc), rk, rv))
            assert torch.equal(outs[0][0], outs[1][0])
            for x, y in ((outs[0][1], outs[1][1]), (outs[0][2], outs[1][2])):
                if f8:
                    assert torch.equal(x.codes, y.codes) and torch.equal(x.scales, y.scales)
                else:  # bit for bit (the poison is NaN)
                    assert torch.equal(x.view(torch.int16), y.view(torch.int16))
        for nh, nkv, D in ((32, 8, 128), (16, 4, 64)):
            case = ap.decode_case(nh, nkv, D, ctxs=ctxs, rows=2)
            a = case.to(DEV)
            kc, vc = _caches(case, a, f8)
            qb = _qblocks(case)
            op = ops.attention_mfma_f8 if f8 else ops.attention_mfma
            for kw in ({}, dict(part_size=128, num_parts=3), dict(part_size=384, num_parts=1)):
                o0 = op(a["q"], kc, vc, *_args(a), qb, nh, nkv, case.scale, **mc, **kw)
                o1 = op(a["q"], kc, vc, *_args(a), qb, nh, nkv, case.scale, window=W, **mc, **kw)
                assert torch.equal(o0, o1), (W, nh, kw)
            rc = ap.rope_case(nh, nkv, D, ctxs=ctxs)
            rop = ops.attention_mfma_rope_f8 if f8 else ops.attention_mfma_rope
            outs = []
            for w_ in (0, W):
                ra = rc.to(DEV)
                rk, rv = _caches(rc, ra, f8)
                outs.append(rop(ra["q"], rk, rv, *_args(ra), _qblocks(rc), ra["positions"], ra["cos"], ra["sin"],
                                ra["slots"], nh, nkv, rc.scale, window=w_, part_size=128, num_parts=3, **mc))
            assert torch.equal(outs[0], outs[1])


# ------------------------------------------------------------------------------------ random inputs
def _random_case(nh, nkv, D, ctxs, seed=0):
    g = torch.Generator().manual_seed(seed)
    npg = [math.ceil(c / 64) for c in ctxs]
    P = sum(npg) + 2
    perm = torch.randperm(P, generator=g).tolist()
    kc = torch.randn(P, nkv, 64, D, generator=g).to(torch.bfloat16)
    vc = torch.randn(P, nkv, 64, D, generator=g).to(torch.bfloat16)
    bt = torch.full((len(ctxs), max(npg)), perm[-1], dtype=torch.int32)
    used, slots = 0, []
    for i, n in enumerate(npg):
        bt[i, :n] = torch.tensor(perm[used:used + n], dtype=torch.int32)
        slots.append(int(bt[i, (ctxs[i] - 1) // 64]) * 64 + (ctxs[i] - 1) % 64)
        used += n
    qkv = torch.randn(len(ctxs), (nh + 2 * nkv) * D, generator=g).to(torch.bfloat16)
    q_seq = torch.arange(len(ctxs), dtype=torch.int32)
    q_ctx = torch.tensor(ctxs, dtype=torch.int32)
    cos, sin = ops.rope_cos_sin(D, max(ctxs) + 1, 10000.0, "cpu")
    return dict(qkv=qkv, kc=kc, vc=vc, bt=bt, q_seq=q_seq, q_ctx=q_ctx, pos=q_ctx.long() - 1,
                slots=torch.tensor(slots, dtype=torch.int64), cos=cos.float(), sin=sin.float())


@pytest.mark.parametrize("kernel", ["paged_attention", "paged_attention_rope", "attention_mfma", "attention_mfma_rope"])
@pytest.mark.parametrize("f8", [False, True])
def test_window_random_inputs_match_the_reference(kernel, f8):
    """randn inputs, W = 100, contexts on both sides of the window: against ``ops.reference`` with the
    window at the attention tolerance of test_kernels_gpu.py."""
    nh, nkv, D = (32, 8, 128) if "mfma" in kernel else (8, 2, 128)
    W, ctxs = 100, [1, 37, 100, 101, 164, 333, 1500]
    c = _random_case(nh, nkv, D, ctxs)
    rope = kernel.endswith("rope")
    # the reference on the CPU, on the cache the kernel reads (fp8: its dequantized values)
    if f8:
        kr, vr = ops.KVF8.from_dense(c["kc"]), ops.KVF8.from_dense(c["vc"])
    else:
        kr, vr = c["kc"].clone(), c["vc"].clone()
    q = c["qkv"].clone()
    if rope:
        (ref.rope_kv_write_f8 if f8 else ref.rope_kv_write)(q, c["pos"], c["cos"], c["sin"], kr, vr, c["slots"], nh, nkv)
    want = (ref.paged_attention_f8 if f8 else ref.paged_attention)(q, kr, vr, c["bt"], c["q_seq"], c["q_ctx"], nh, nkv,
                                                                   1 / math.sqrt(D), window=W)
    d = {k: v.to(DEV) for k, v in c.items()}
    if f8:
        kc, vc = (ops.KVF8(x.codes.to(DEV), x.scales.to(DEV)) for x in (ops.KVF8.from_dense(c["kc"]),
                                                                        ops.KVF8.from_dense(c["vc"])))
    else:
        kc, vc = d["kc"], d["vc"]
    meta = (d["bt"], d["q_seq"], d["q_ctx"])
    ropeargs = (d["pos"], d["cos"], d["sin"], d["slots"])
    qb = torch.from_numpy(ops.query_blocks([1] * len(ctxs), nh // nkv)).to(DEV)
    sc = 1 / math.sqrt(D)
    if kernel == "paged_attention":
        out = ops.paged_attention(d["qkv"], kc, vc, *meta, nh, nkv, sc, window=W)
    elif kernel == "paged_attention_rope":
        out = ops.paged_attention_rope(d["qkv"], kc, vc, *meta, *ropeargs, nh, nkv, sc, window=W)
    elif kernel == "attention_mfma":
        out = (ops.attention_mfma_f8 if f8 else ops.attention_mfma)(d["qkv"], kc, vc, *meta, qb, nh, nkv, sc, window=W)
    else:
        out = (ops.attention_mfma_rope_f8 if f8 else ops.attention_mfma_rope)(d["qkv"], kc, vc, *meta, qb, *ropeargs, nh,
                                                                              nkv, sc, window=W)
    torch.testing.assert_close(out.float().cpu(), want.float(), atol=2e-2, rtol=2e-2)


# ------------------------------------------------------------------------------------ rejections
def test_launches_without_a_windowed_form_refuse_a_window():
    nh, nkv, D = 8, 2, 128
    case = ap.prefill_case(nh, nkv, D, [130], [0])
    a = case.to(DEV)
    args = (a["q"], a["k_cache"], a["v_cache"], *_args(a))
    fb = torch.from_numpy(ops.fa_blocks([130], nh // nkv, 4)).to(DEV)
    qb = torch.from_numpy(ops.query_blocks([130], nh // nkv)).to(DEV)
    sb = torch.from_numpy(ops.query_superblocks([130], nh // nkv)).to(DEV)
    ops.attention_fa(*args, fb, nh, nkv, case.scale, waves=4)  # (the same launches without a window run)
    ops.attention_mfma(*args, qb, nh, nkv, case.scale, superblocks=sb)
    with pytest.raises(RuntimeError, match="sliding-window"):
        ops.attention_fa(*args, fb, nh, nkv, case.scale, waves=4, window=64)
    kf, vf = case.f8(DEV)
    with pytest.raises(RuntimeError, match="sliding-window"):
        ops.attention_fa_f8(a["q"], kf, vf, *_args(a), fb, nh, nkv, case.scale, waves=4, window=64)
    with pytest.raises(RuntimeError, match="sliding-window"):
        ops.attention_mfma(*args, qb, nh, nkv, case.scale, superblocks=sb, window=64)
    with pytest.raises(RuntimeError, match="sliding-window"):  # multi-token blocks of the one-block kernel
        ops.attention_mfma(*args, qb, nh, nkv, case.scale, window=64)


# ------------------------------------------------------------------------------------ executor
def _fake_quant_hook(k, v):
    return ops.fake_quant_kv_fp8(k), ops.fake_quant_kv_fp8(v)


def _cfg(kind):
    base = dataclasses.replace(resolve_model("tiny-llama"), model_type="mistral", sliding_window=96)
    if kind == "flash":  # nh / nkv = 2: decode on the flash-decoding kernel
        return base
    # nh / nkv = 4, head_dim 64: decode on the MFMA GQA kernel
    return dataclasses.replace(base, num_attention_heads=8, num_key_value_heads=2, hidden_size=512)


@functools.lru_cache(maxsize=None)
def _weights(kind):
    cfg = _cfg(kind)
    return random_stage_weights(cfg, 0, cfg.num_hidden_layers, has_embed=True, has_head=True, device=DEV,
                                dtype=torch.bfloat16, seed=4)


@pytest.mark.parametrize("kind", ["flash", "mfma"])
@pytest.mark.parametrize("kv", ["bf16", "fp8"])
@pytest.mark.parametrize("graphs", [False, True])
def test_executor_attends_past_the_window(kind, kv, graphs):
    """Prompts of 80 and 9 tokens decoded until both sessions are past 3 W: logits against the windowed
    fp32 oracle every 16th step (bound of test_mixtral_gpu_matches_fp32_reference), held pages within
    ceil(W / 64) + 1, and with graphs no new capture once both sessions are past the window."""
    cfg, w = _cfg(kind), _weights(kind)
    W = cfg.sliding_window
    ex = StageExecutor(cfg, w, DEV, kv_cache_bytes=64 << 20, max_sessions=4, use_graphs=graphs, kv_cache_dtype=kv,
                       sliding_window="attend")
    assert ex.window == W and ex.max_seq_len == cfg.max_position_embeddings
    assert (ex.gqa_decode_mfma or ex.gqa_decode_mfma_f8) == (kind == "mfma")
    hook = _fake_quant_hook if kv == "fp8" else None
    g = torch.Generator().manual_seed(0)
    seqs = [torch.randint(0, cfg.vocab_size, (n,), generator=g) for n in (80, 9)]
    logits = ex.forward([("a", 80), ("b", 9)], torch.cat(seqs).to(DEV))
    bound = math.ceil(W / 64) + 1
    step, graphs_past = 0, None
    while True:
        if step % 16 == 0:
            for i, p in enumerate(seqs):
                want = reference_forward([w], p.to(DEV), kv_hook=hook, window=W)[-1]
                torch.testing.assert_close(logits[i].float(), want, atol=0.06, rtol=0.05)
        for sid in ("a", "b"):
            assert len(ex.sessions.get(sid).pages) <= bound
        if min(len(p) for p in seqs) > 3 * W:
            break
        if graphs and graphs_past is None and min(len(p) for p in seqs) > W + 31:
            graphs_past = len(ex._graphs)
        nxt = torch.argmax(logits.float(), -1)
        seqs = [torch.cat([s, nxt[i:i + 1].cpu()]) for i, s in enumerate(seqs)]
        logits = ex.forward([("a", 1), ("b", 1)], nxt)
        step += 1
        assert ex.last_graphed == graphs
    assert ex.sessions.get("a").first_page > 0 and ex.sessions.get("b").first_page > 0
    if graphs:
        assert graphs_past is not None and len(ex._graphs) == graphs_past


def test_executor_prefill_past_the_window_runs_the_windowed_rows():
    """A 250-token prompt (max_ctx > W) and a chunked one: the prefill steps past the window run the
    flash-decoding kernel with the window and match the windowed oracle."""
    cfg, w = _cfg("flash"), _weights("flash")
    W = cfg.sliding_window
    ids = torch.randint(0, cfg.vocab_size, (250,), generator=torch.Generator().manual_seed(5))
    want = reference_forward([w], ids.to(DEV), window=W)[-1]
    for kw in ({}, dict(max_tokens_per_step=64)):
        ex = StageExecutor(cfg, w, DEV, kv_cache_bytes=64 << 20, max_sessions=2, use_graphs=False,
                           sliding_window="attend", **kw)
        lg = ex.forward([("s", 250)], ids.to(DEV))
        torch.testing.assert_close(lg[0].float(), want, atol=0.06, rtol=0.05)
        assert len(ex.sessions.get("s").pages) <= math.ceil(W / 64) + 1
