"""Host-side argument checks of the attention and KV-write ops (ops/csrc/bindings.cpp): each of
``rope_kv_write``, ``rope_kv_write_f8``, ``kv_write``, ``paged_attention``, ``paged_attention_f8``,
``paged_attention_rope``, ``paged_attention_rope_f8``, ``attention_mfma``, ``attention_mfma_rope`` and
``attention_fa`` rejects one bad argument at a time with the message the op has always raised, before any
kernel is launched; one valid call per op gives the bits (and the cache writes) of its ``ops.*`` wrapper.
An ``_f8`` entry is the fp8-cache form of its base torch op: the same op with ``k_scale`` / ``v_scale``.

The shape is the smallest one all three kernels and the fp8 cache accept: 2 decode tokens with contexts
5 and 9, 4 query heads on 2 kv heads, head_dim 128, 64-token pages, one page per sequence out of a pool
of 3, one 128-token context part.  A rule on a derived size (the head dim, the page size) is reached
with a full argument set built for that size, so that it is the only rule broken."""
import re

import pytest
import torch

from src import ops

pytestmark = pytest.mark.gpu
DEV = "cuda"
T, NH, NKV, PAGE, POOL = 2, 4, 2, 64, 3
CTX = [5, 9]
PART, NPARTS = 128, 1

F8_OPS = ("rope_kv_write_f8", "paged_attention_f8", "paged_attention_rope_f8")
ROPE_ATTN = ("paged_attention_rope", "paged_attention_rope_f8", "attention_mfma_rope")
ROPE_OPS = ("rope_kv_write", "rope_kv_write_f8") + ROPE_ATTN
PAGED = ("paged_attention", "paged_attention_f8", "paged_attention_rope", "paged_attention_rope_f8")
ATTN = PAGED + ("attention_mfma", "attention_mfma_rope", "attention_fa")
ALL_OPS = ("rope_kv_write", "rope_kv_write_f8", "kv_write") + ATTN
# the launcher an op ends in: the name in "<launcher> launch failed with code N"
LAUNCHER = {"paged_attention_rope": "paged_attention", "paged_attention_rope_f8": "paged_attention_f8",
            "attention_mfma_rope": "attention_mfma"}

COS_SIN = "cos/sin tables fp32 [max_pos, D/2]"
CACHE4 = "cache [pages, nkv, page, D]"
F8_TENSORS = "fp8 KV cache: codes and scales are contiguous uint8 tensors on one GPU"
F8_CODES = "fp8 KV codes [pages, nkv, page, D]"
F8_HEAD_DIM = "fp8 KV cache: head_dim 64 or 128"
F8_SCALES = "fp8 KV scales [pages, nkv, page] must match the codes' pages, heads and page_size"
F8_ALIGNED = "fp8 KV codes must be 8-B aligned"
QKV_PART = "qkv_part: fp32 [S, T, qkv width] split-K slabs (ops.linear_partials)"
PART_SS = "part_ss: row statistics [32, 256] int64"
COUNTERS = "counters: zero-initialised cuda int32"
QBLOCKS = "qblocks int32 [2, NB] (first token, token count)"
SUPERBLOCKS = "superblocks int32 [2, NSB] (ops.query_superblocks)"
FABLOCKS = "fablocks int32 [2, NB] (first token, token count), ops.fa_blocks"
MX_OUT = "mx output: packed, one part, D 128, as_"


@pytest.fixture(scope="module", autouse=True)
def _native():
    ops.require_native()


def _torch_op(op):
    """The torch op of a table entry: an ``_f8`` entry is its base op called with ``k_scale`` / ``v_scale``."""
    return getattr(torch.ops.mpamd, op.removesuffix("_f8"))


def _bf(*shape):
    return torch.zeros(*shape, dtype=torch.bfloat16, device=DEV)


def _u8(*shape):
    return torch.zeros(*shape, dtype=torch.uint8, device=DEV)


def _i32(x):
    return torch.as_tensor(x, dtype=torch.int32).to(DEV)


def _strided(t):
    """``t``'s shape and dtype with twice the inner pitch: not contiguous."""
    return t.new_zeros(*t.shape[:-1], 2 * t.shape[-1])[..., : t.shape[-1]]


def _off_by_one(t):
    """``t``'s shape and dtype, contiguous, one element past an aligned address."""
    return t.new_zeros(t.numel() + 8)[1:1 + t.numel()].view(t.shape)


def _args(op, D=128, page=PAGE):
    """Valid keyword arguments of ``torch.ops.mpamd.<op>`` on random data (the same for every op)."""
    torch.manual_seed(D + page)
    W, WQKV = NH * D, (NH + 2 * NKV) * D
    kd = torch.randn(POOL, NKV, page, D, device=DEV).to(torch.bfloat16)
    vd = torch.randn(POOL, NKV, page, D, device=DEV).to(torch.bfloat16)
    qkv = torch.randn(T, WQKV, device=DEV).to(torch.bfloat16)
    bt = _i32([[2], [0]])
    pos = torch.tensor([c - 1 for c in CTX], device=DEV)
    cos, sin = ops.rope_cos_sin(D, 16, 10000.0, DEV)
    a = dict(k_cache=kd, v_cache=vd)
    if op in F8_OPS:
        kf, vf = ops.KVF8.from_dense(kd), ops.KVF8.from_dense(vd)
        a = dict(k_cache=kf.codes, v_cache=vf.codes, k_scale=kf.scales, v_scale=vf.scales)
    if op == "kv_write":
        k, v = qkv[:, W:W + NKV * D], qkv[:, W + NKV * D:]
        return a | dict(k=k, v=v, slots=bt[:, 0].long() * page + pos)
    if op in ROPE_OPS:
        a.update(qkv=qkv, positions=pos, cos=cos, sin=sin, slots=bt[:, 0].long() * page + pos, nh=NH, nkv=NKV)
        if op not in ROPE_ATTN:
            return a
    else:
        a.update(q=qkv[:, :W].contiguous(), nh=NH, nkv=NKV)
    a.update(block_tables=bt, q_seq=_i32([0, 1]), q_ctx=_i32(CTX), out=_bf(T, W),
             workspace=ops.attention_workspace(T, NH, D, NPARTS, DEV), scale=D ** -0.5, part_size=PART,
             num_parts=NPARTS)
    if op == "attention_fa":
        return a | dict(fablocks=_i32(ops.fa_blocks([1] * T, NH // NKV, 4)), waves=4, pair=0)
    a.update(packed=0)
    if op in ("attention_mfma", "attention_mfma_rope"):
        a.update(qblocks=_i32(ops.query_blocks([1] * T, NH // NKV)))
    return a


def _row_cases(arg, name, t):
    """The bf16 row-major operand rules of argument ``arg``, called ``name`` in the messages."""
    r, w = t.shape
    return [(f"{name} must be on the GPU", {arg: t.cpu()}),
            (f"{name} must be bf16", {arg: t.half()}),
            (f"{name} must be 2-D [rows, cols]", {arg: t[:, :, None]}),
            (f"{name} must have unit inner stride", {arg: t.new_zeros(r, 2 * w)[:, ::2]}),
            (f"{name} row stride must be a multiple of 8", {arg: t.new_zeros(r, w + 4)[:, :w]}),
            (f"{name} must be 16-B aligned", {arg: _off_by_one(t)})]


def _index_cases(arg, msg, t, contiguous=True):
    """An index vector of T entries: its dtype, its length and (where the op asks) its contiguity."""
    other = torch.int32 if t.dtype == torch.int64 else torch.int64
    cases = [(msg, {arg: t.to(other)}), (msg, {arg: t.new_zeros(T + 1)})]
    if contiguous:
        cases.append((msg, {arg: t.new_zeros(2 * T)[::2]}))
    return cases


def _bf16_cache_cases(a):
    return [("k_cache must be on the GPU", dict(k_cache=a["k_cache"].cpu())),
            ("k_cache must be bf16", dict(k_cache=a["k_cache"].half())),
            ("v_cache must be on the GPU", dict(v_cache=a["v_cache"].cpu())),
            ("v_cache must be bf16", dict(v_cache=a["v_cache"].half())),
            (CACHE4, dict(k_cache=a["k_cache"][0]))]


def _f8_cache_cases(op, a):
    cases = [(F8_TENSORS, dict(k_scale=a["k_scale"].to(torch.int8))),
             (F8_TENSORS, dict(v_cache=_strided(a["v_cache"]))),
             (F8_TENSORS, dict(v_scale=a["v_scale"].cpu())),
             (F8_CODES, dict(v_cache=_u8(POOL + 1, NKV, PAGE, 128))),
             (F8_HEAD_DIM, _args(op, D=32)),
             (F8_SCALES, dict(k_scale=_u8(POOL, NKV, PAGE // 2))),
             (F8_SCALES, dict(k_scale=a["k_scale"][..., None], v_scale=a["v_scale"][..., None])),
             (F8_ALIGNED, dict(k_cache=_off_by_one(a["k_cache"]))),
             (F8_ALIGNED, dict(v_cache=_off_by_one(a["v_cache"])))]
    if op == "paged_attention_f8":
        cases.append((F8_CODES, dict(nkv=1)))
    if op == "rope_kv_write_f8":
        cases.append((F8_CODES, dict(nh=NH + 2, nkv=1)))  # (the same qkv width)
    return cases


def _rope_cases(op, a):
    w = a["qkv"].shape[1]
    cases = [("qkv width", dict(qkv=_bf(T, w + 8)))]
    cases += _index_cases("positions", "positions", a["positions"])
    cases += _index_cases("slots", "slots", a["slots"])
    cases += [(COS_SIN, dict(cos=a["cos"].half())),
              (COS_SIN, dict(sin=a["sin"].double())),
              (COS_SIN, dict(cos=_strided(a["cos"]))),
              (COS_SIN, dict(sin=_strided(a["sin"]))),
              (COS_SIN, dict(cos=a["cos"][:, :-1].contiguous())),
              (COS_SIN, dict(sin=a["sin"][:-1]))]
    if op == "paged_attention_rope":
        cases.append(("head dim", _args(op, D=72)))
    return cases


def _qkv_part_cases(a):
    w = a["qkv"].shape[1]
    part = torch.zeros(2, T, w, device=DEV)
    ss = ops.norm_stats_buffer(DEV)[0]
    qp = dict(qkv_part=part, part_splits=2, part_ss=ss, inv_k=1.0 / 4096, eps=1e-5)
    return [(QKV_PART, qp | dict(qkv_part=part.cpu())),
            (QKV_PART, qp | dict(qkv_part=part.double())),
            (QKV_PART, qp | dict(qkv_part=_strided(part))),
            (QKV_PART, qp | dict(qkv_part=part[0])),
            (QKV_PART, qp | dict(part_splits=3)),
            (QKV_PART, qp | dict(qkv_part=part[:, :1].contiguous())),
            (QKV_PART, qp | dict(qkv_part=part[:, :, 8:].contiguous())),
            ("qkv_part splits", qp | dict(qkv_part=torch.zeros(9, T, w, device=DEV), part_splits=9)),
            ("qkv_part splits", qp | dict(qkv_part=part[:0], part_splits=0)),
            (PART_SS, qp | dict(part_ss=ss.cpu())),
            (PART_SS, qp | dict(part_ss=ss.int())),
            (PART_SS, qp | dict(part_ss=ss.view(-1)[:-1])),
            (PART_SS, qp | dict(part_ss=ss.new_zeros(2 * ss.numel())[::2]))]


def _attention_cases(op, a):
    """The operand rules every attention op shares, and the launcher's own shape rule."""
    qn = "qkv" if op in ROPE_ATTN else "q"
    D = a["k_cache"].shape[3]
    W = NH * D
    cases = _row_cases(qn, "q", a[qn])
    cases += [("out must be on the GPU", dict(out=a["out"].cpu())),
              ("out must be bf16", dict(out=a["out"].half())),
              ("out contiguous", dict(out=_strided(a["out"]))),
              ("out numel", dict(out=_bf(T, W + 8))),
              ("block_tables int32 [S, max_pages]", dict(block_tables=a["block_tables"].long())),
              ("block_tables int32 [S, max_pages]", dict(block_tables=a["block_tables"][:, 0])),
              ("block_tables int32 [S, max_pages]", dict(block_tables=a["block_tables"].new_zeros(T, 2)[:, ::2])),
              ("workspace fp32", dict(workspace=a["workspace"].half())),
              ("workspace too small", dict(num_parts=2, workspace=torch.zeros(T * NH * 2 * (D + 2) - 1, device=DEV))),
              (f"{LAUNCHER.get(op, op)} launch failed with code -1", dict(part_size=96))]
    cases += _index_cases("q_seq", "q_seq", a["q_seq"], contiguous=False)
    cases += _index_cases("q_ctx", "q_ctx", a["q_ctx"], contiguous=False)
    if op not in ROPE_ATTN:  # (the fused ops' qkv width leaves q no way to be too narrow)
        cases.append(("q width", dict(q=_bf(T, W - 8))))
    if op != "attention_fa":
        cases.append(("packed out numel", dict(packed=1, out=_bf(ops.packed_numel(T, W) - 1))))
    if op in F8_OPS:
        cases += _f8_cache_cases(op, a)
    else:
        cases += _bf16_cache_cases(a)
        cases += [(CACHE4, dict(v_cache=_bf(POOL + 1, NKV, PAGE, 128))),
                  ("cache", dict(k_cache=_strided(a["k_cache"]))), ("cache", dict(v_cache=_strided(a["v_cache"])))]
        if op not in ROPE_ATTN:
            cases.append(("cache", dict(nkv=1)))
    if op in PAGED:
        cnt = torch.zeros(64, dtype=torch.int32, device=DEV)
        cases += [(COUNTERS, dict(counters=cnt.cpu())), (COUNTERS, dict(counters=cnt.long())),
                  (COUNTERS, dict(counters=cnt[::2]))]
    if op in ("paged_attention", "paged_attention_f8", "attention_mfma"):  # a page size that is no power of two
        cases.append((f"{op} launch failed with code -2", _args(op, page=96)))
    return cases


def _bad_cases(op):
    """(message, changed arguments) pairs: each violates exactly one check of ``op``."""
    a = _args(op)
    if op == "kv_write":
        w = NKV * 128
        return (_row_cases("k", "k", a["k"]) + _row_cases("v", "v", a["v"])
                + _index_cases("slots", "slots", a["slots"], contiguous=False)
                + [("cache layout", dict(k_cache=a["k_cache"][0])),
                   ("cache layout", dict(k_cache=_strided(a["k_cache"]))),
                   ("cache layout", dict(v_cache=_strided(a["v_cache"]))),
                   ("k/v width", dict(k=_bf(T, w - 8))),
                   ("k/v width", dict(v=_bf(T, w + 8)))])
    if op == "rope_kv_write":
        return (_row_cases("qkv", "qkv", a["qkv"]) + _bf16_cache_cases(a) + _rope_cases(op, a)
                + [(CACHE4, dict(k_cache=_strided(a["k_cache"]))),
                   (CACHE4, dict(v_cache=_strided(a["v_cache"]))),
                   ("k/v cache shapes differ", dict(v_cache=_bf(POOL + 1, NKV, PAGE, 128))),
                   ("cache kv heads", dict(nh=NH + 2, nkv=1))])  # (the same qkv width)
    if op == "rope_kv_write_f8":
        return _row_cases("qkv", "qkv", a["qkv"]) + _f8_cache_cases(op, a) + _rope_cases(op, a)
    cases = _attention_cases(op, a)
    if op in ROPE_ATTN:
        cases += _rope_cases(op, a) + _qkv_part_cases(a)
    if op in ("attention_mfma", "attention_mfma_rope"):
        qb = a["qblocks"]
        cases += [(QBLOCKS, dict(qblocks=qb.long())), (QBLOCKS, dict(qblocks=qb.new_zeros(3, T))),
                  (QBLOCKS, dict(qblocks=_strided(qb)))]
    if op == "attention_mfma":
        cases.append((QBLOCKS, dict(qblocks=qb[0])))
        sb = _i32(ops.query_superblocks([1] * T, NH // NKV))
        cases += [(SUPERBLOCKS, dict(superblocks=sb.cpu())), (SUPERBLOCKS, dict(superblocks=sb.long())),
                  (SUPERBLOCKS, dict(superblocks=sb.new_zeros(3, T))), (SUPERBLOCKS, dict(superblocks=_strided(sb))),
                  (SUPERBLOCKS, dict(superblocks=sb.new_zeros(2, T + 1)))]
    if op == "attention_mfma_rope":
        W = NH * 128
        mx = dict(packed=1, out=_bf(ops.packed_numel(T, W)), mx_ax=_u8(16 * W), mx_as=_u8(2 * W))
        cases += [("fused RoPE needs one query token per block (decode)", dict(qblocks=a["qblocks"][:, :1].contiguous())),
                  (MX_OUT, mx | dict(mx_as=None)),
                  (MX_OUT, mx | dict(packed=0, out=a["out"])),
                  (MX_OUT, mx | dict(num_parts=2, workspace=ops.attention_workspace(T, NH, 128, 2, DEV))),
                  ("mx_ax: uint8 [ceil(T/16)*16*K]", mx | dict(mx_ax=_u8(16 * W - 1))),
                  ("mx_ax: uint8 [ceil(T/16)*16*K]", mx | dict(mx_ax=mx["mx_ax"].to(torch.int8))),
                  ("mx_ax: uint8 [ceil(T/16)*16*K]", mx | dict(mx_ax=mx["mx_ax"].cpu())),
                  ("mx_as: uint8 [2K]", mx | dict(mx_as=_u8(2 * W - 1))),
                  ("mx_as: uint8 [2K]", mx | dict(mx_as=_u8(4 * W)[::2]))]
    if op == "attention_fa":
        fb = a["fablocks"]
        cases += [(FABLOCKS, dict(fablocks=fb.cpu())), (FABLOCKS, dict(fablocks=fb.long())),
                  (FABLOCKS, dict(fablocks=fb.new_zeros(3, T))), (FABLOCKS, dict(fablocks=fb[0])),
                  (FABLOCKS, dict(fablocks=_strided(fb))),
                  ("waves 4 or 8", dict(waves=5)),
                  ("attention_fa: head_dim 128", _args(op, D=64))]
    return cases


@pytest.mark.parametrize("op", ALL_OPS)
def test_one_bad_argument_is_rejected_with_its_message(op):
    fn = _torch_op(op)
    a = _args(op)
    for msg, change in _bad_cases(op):
        with pytest.raises(RuntimeError, match=re.escape("mpamd: " + msg) + r"(\n|$)"):
            fn(**(a | change))


def _f8_args(op):
    """``_args(op)`` of an MFMA op on the fp8 cache of the same data."""
    a = _args(op)
    kf, vf = ops.KVF8.from_dense(a["k_cache"]), ops.KVF8.from_dense(a["v_cache"])
    return a | dict(k_cache=kf.codes, v_cache=vf.codes, k_scale=kf.scales, v_scale=vf.scales)


ONE_SCALE = "fp8 KV cache: k_scale and v_scale are given together (neither: a bf16 cache)"
F8_SUPERBLOCKS = "attention_mfma on an fp8 KV cache has no grouped prefill form: superblocks must be None"
F8_MX_OUT = "attention_mfma on an fp8 KV cache has no MX output: mx_ax must be None"


def _scale_cases(rule):
    """(op, message, arguments) of the rules the trailing ``k_scale`` / ``v_scale`` bring."""
    if rule == "one_scale":  # on every merged op, from its fp8 call and from its bf16 call
        cases = []
        for op in F8_OPS:
            a = _args(op)
            cases += [(op, ONE_SCALE, a | dict(k_scale=None)), (op, ONE_SCALE, a | dict(v_scale=None))]
        for op in ("attention_mfma", "attention_mfma_rope", "attention_fa"):
            a = _args(op)
            s = ops.KVF8.from_dense(a["k_cache"]).scales
            cases += [(op, ONE_SCALE, a | dict(k_scale=s)), (op, ONE_SCALE, a | dict(v_scale=s))]
        return cases
    if rule == "superblocks":
        sb = _i32(ops.query_superblocks([1] * T, NH // NKV))
        return [("attention_mfma", F8_SUPERBLOCKS, _f8_args("attention_mfma") | dict(superblocks=sb))]
    W = NH * 128
    mx = dict(packed=1, out=_bf(ops.packed_numel(T, W)), mx_ax=_u8(16 * W), mx_as=_u8(2 * W))
    return [("attention_mfma_rope", F8_MX_OUT, _f8_args("attention_mfma_rope") | mx)]


@pytest.mark.parametrize("rule", ["one_scale", "superblocks", "mx_ax"])
def test_scale_arguments_refuse_what_no_kernel_form_covers(rule):
    """One scale tensor without the other, and the two MFMA forms a bf16 cache alone has - superblocks
    and the MX output - with scales: raised before any launch (the zeroed output stays zero)."""
    for op, msg, a in _scale_cases(rule):
        with pytest.raises(RuntimeError, match=re.escape("mpamd: " + msg) + r"(\n|$)"):
            _torch_op(op)(**a)
        if "out" in a:
            torch.cuda.synchronize()
            assert not bool(a["out"].any())


# ----------------------------------------------------------------------------------------- valid calls
def _caches(a):
    """The wrapper's cache arguments of the op arguments ``a`` (``KVF8`` pairs on an fp8 cache)."""
    if "k_scale" in a:
        return ops.KVF8(a["k_cache"], a["k_scale"]), ops.KVF8(a["v_cache"], a["v_scale"])
    return a["k_cache"], a["v_cache"]


WRITTEN = ("qkv", "k_cache", "v_cache", "k_scale", "v_scale")


def _cloned(a):
    """``a`` with its own copy of everything a cache-writing op writes."""
    return {k: (v.clone() if k in WRITTEN else v) for k, v in a.items()}


def _same_writes(a, b):
    return all(torch.equal(a[k], b[k]) for k in WRITTEN if k in a)


@pytest.mark.parametrize("op", ["rope_kv_write", "rope_kv_write_f8"])
def test_rope_kv_write_valid_call_equals_wrapper(op):
    base = _args(op)
    a, b = _cloned(base), _cloned(base)
    _torch_op(op)(**a)
    ops.rope_kv_write(b["qkv"], b["positions"], b["cos"], b["sin"], *_caches(b), b["slots"], NH, NKV)
    assert _same_writes(a, b)
    assert not torch.equal(a["k_cache"], base["k_cache"]) and not torch.equal(a["qkv"], base["qkv"])


def test_kv_write_valid_call_equals_wrapper():
    base = _args("kv_write")
    a, b = _cloned(base), _cloned(base)
    torch.ops.mpamd.kv_write(**a)
    ops.kv_write(b["k"], b["v"], b["k_cache"], b["v_cache"], b["slots"])
    assert _same_writes(a, b)
    assert not torch.equal(a["v_cache"], base["v_cache"])


@pytest.mark.parametrize("op", ["paged_attention", "paged_attention_f8"])
def test_paged_attention_valid_call_equals_wrapper(op):
    a = _args(op)
    _torch_op(op)(**a)
    want = ops.paged_attention(a["q"], *_caches(a), a["block_tables"], a["q_seq"], a["q_ctx"], NH, NKV, a["scale"],
                               part_size=PART, num_parts=NPARTS)
    assert torch.equal(a["out"], want) and bool(a["out"].any())


@pytest.mark.parametrize("op", ["paged_attention_rope", "paged_attention_rope_f8"])
def test_paged_attention_rope_valid_call_equals_wrapper(op):
    base = _args(op)
    a, b = _cloned(base), _cloned(base)
    _torch_op(op)(**a)
    want = ops.paged_attention_rope(b["qkv"], *_caches(b), b["block_tables"], b["q_seq"], b["q_ctx"], b["positions"],
                                    b["cos"], b["sin"], b["slots"], NH, NKV, b["scale"], part_size=PART,
                                    num_parts=NPARTS)
    assert torch.equal(a["out"], want) and bool(a["out"].any())
    assert _same_writes(a, b)
    assert not torch.equal(a["k_cache"], base["k_cache"]) and torch.equal(a["qkv"], base["qkv"])


def test_attention_mfma_valid_call_equals_wrapper():
    a = _args("attention_mfma")
    torch.ops.mpamd.attention_mfma(**a)
    want = ops.attention_mfma(a["q"], a["k_cache"], a["v_cache"], a["block_tables"], a["q_seq"], a["q_ctx"],
                              a["qblocks"], NH, NKV, a["scale"], part_size=PART, num_parts=NPARTS)
    assert torch.equal(a["out"], want) and bool(a["out"].any())


def test_attention_mfma_rope_valid_call_equals_wrapper():
    base = _args("attention_mfma_rope")
    a, b = _cloned(base), _cloned(base)
    torch.ops.mpamd.attention_mfma_rope(**a)
    want = ops.attention_mfma_rope(b["qkv"], b["k_cache"], b["v_cache"], b["block_tables"], b["q_seq"], b["q_ctx"],
                                   b["qblocks"], b["positions"], b["cos"], b["sin"], b["slots"], NH, NKV, b["scale"],
                                   part_size=PART, num_parts=NPARTS)
    assert torch.equal(a["out"], want) and bool(a["out"].any())
    assert _same_writes(a, b)
    assert not torch.equal(a["k_cache"], base["k_cache"]) and torch.equal(a["qkv"], base["qkv"])


def test_attention_fa_valid_call_equals_wrapper():
    a = _args("attention_fa")
    torch.ops.mpamd.attention_fa(**a)
    # (max_ctx = 128 in one part: the wrapper derives part_size 128, the direct call's)
    want = ops.attention_fa(a["q"], a["k_cache"], a["v_cache"], a["block_tables"], a["q_seq"], a["q_ctx"],
                            a["fablocks"], NH, NKV, a["scale"], max_ctx=PART, waves=4, num_parts=NPARTS, pair=False)
    assert torch.equal(a["out"], want) and bool(a["out"].any())
