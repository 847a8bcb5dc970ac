"""CPU self-test of the attention probes (tests/attn_probe.py): the closed form is right, the values
are exact in bf16 and fp8, the reference ops pass the comparator, and - what makes the GPU probes
worth having - a dense fp64 attention with one deliberate mistake (a dropped key, a visible trap, a
key counted twice, a split-K slice left out, a stale cache slot) is rejected on EVERY probe row
that depends on the mistaken key."""
import functools
import math

import pytest
import torch

from src import ops
from tests import attn_probe as ap

DECODE_SHAPES = [(8, 2, 128), (32, 8, 128), (12, 12, 64), (8, 2, 64)]


@functools.lru_cache(maxsize=None)
def _decode(nh, nkv, D, short=False):
    return ap.decode_case(nh, nkv, D, short_ctx=short)


@functools.lru_cache(maxsize=None)
def _rope(nh, nkv, D, quarter=False):
    return ap.rope_case(nh, nkv, D, quarter=quarter)


@functools.lru_cache(maxsize=None)
def _prefill(nh, nkv, D):
    return ap.prefill_case(nh, nkv, D, [300, 17], [64, 5])


def dense(case, t, drop=(), trap=False, twice=None, part=None, skip=None, v_override=None, q=None):
    """fp64 attention of query row t over its sequence's gathered K / V as split-K partials (m, l, o)
    of ``part``-token slices combined in slice order, with optional mistakes: ``drop`` keys made
    invisible, the ``trap`` (position ctx) visible, key ``twice`` counted twice, slice ``skip`` left
    out of the combine, ``v_override`` = (position, V [nkv, D]) read instead of the cached row.
    ``q`` [nh, D] replaces the row's own q (the rotated q of a RoPE case).
    Returns (out [nh, D], weights [nh, ctx + 1])."""
    seq = case.seqs[int(case.q_seq[t])]
    c = int(case.q_ctx[t])
    nh, nkv, D = case.nh, case.nkv, case.D
    K, V = seq.K[: c + 1], seq.V[:, : c + 1].clone()
    if v_override is not None:
        V[:, v_override[0]] = v_override[1]
    V = V.repeat_interleave(nh // nkv, 0)
    if q is None:
        q = case.q[t, : nh * D].double().view(nh, D)
    s = q @ K.T * case.scale
    vis = torch.arange(c + 1) < c
    vis[c] = trap
    for e in drop:
        vis[e] = False
    if twice is not None:
        s[:, twice] += math.log(2.0)
    s = s.masked_fill(~vis, float("-inf"))
    part = part or c + 1
    ms, ls, os_ = [], [], []
    for i, a in enumerate(range(0, c + 1, part)):
        if i == skip:
            continue
        sl = s[:, a : a + part]
        m = sl.amax(-1)
        p = torch.exp(sl - torch.where(m.isinf(), torch.zeros_like(m), m)[:, None])
        ms.append(m)
        ls.append(p.sum(-1))
        os_.append(torch.einsum("hn,hnd->hd", p, V[:, a : a + part]))
    if not ms:  # the only slice left out: nothing attended to
        return torch.zeros(nh, D, dtype=torch.float64), torch.zeros(nh, c + 1, dtype=torch.float64)
    M = torch.stack(ms).amax(0)
    M = torch.where(M.isinf(), torch.zeros_like(M), M)
    wgt = [torch.exp(m - M) for m in ms]
    den = sum(w * l for w, l in zip(wgt, ls))
    num = sum(w[:, None] * o for w, o in zip(wgt, os_))
    out = torch.where(den[:, None] > 0, num / den.clamp_min(1e-300)[:, None], torch.zeros_like(num))
    return out, torch.softmax(s, -1).nan_to_num(0.0)


def mutated(case, rows, **kw):
    """The bf16 output of a kernel that makes the mistake ``kw`` on ``rows``, exact elsewhere."""
    out = case.expected.clone().view(case.T, case.nh, case.D)
    for t in rows:
        out[t] = dense(case, t, **kw)[0]
    return out.view(case.T, -1).to(torch.bfloat16)


def probe_rows(case):
    return torch.nonzero(case.probe_rows).flatten().tolist()


def assert_rejects(case, out, hit, what):
    """``hit(t, probe)``: the probe depends on the mistake.  Every such (row, head) must be rejected."""
    rej = ap.rejected(out, case)
    n = 0
    for t in probe_rows(case):
        for h, pr in enumerate(case.probes[t]):
            if hit(t, pr):
                n += 1
                assert bool(rej[t, h]), f"{what}: row {t} head {h} {pr} (ctx {int(case.q_ctx[t])}) passed"
    return n


CASES = {"decode-32-8-128": lambda: _decode(32, 8, 128), "decode-12-12-64": lambda: _decode(12, 12, 64),
         "decode-short-8-2-64": lambda: _decode(8, 2, 64, True), "prefill-16-4-128": lambda: _prefill(16, 4, 128),
         "prefill-12-12-64": lambda: _prefill(12, 12, 64), "rope-32-8-128": lambda: _rope(32, 8, 128),
         "rope-quarter-12-12-64": lambda: _rope(12, 12, 64, True)}
ALL_CASES = sorted(CASES)


@pytest.mark.parametrize("mk", ALL_CASES)
def test_reference_equals_closed_form(mk):
    case = CASES[mk]()
    worst, bg = 0.0, 0.0
    for t in probe_rows(case):
        out, p = dense(case, t, **rope_kw(case, t))
        worst = max(worst, float((out - case.expected[t].view(case.nh, case.D)).abs().max()))
        for h, pr in enumerate(case.probes[t]):
            bg = max(bg, float(1.0 - p[h, list(pr.keys)].sum()))
        assert float(p[:, int(case.q_ctx[t])].max()) == 0.0
    assert worst <= 1e-9 and bg <= 1e-6, (worst, bg)
    # a second split (two-slice combine) of the same reference agrees too
    t = probe_rows(case)[-1]
    if case.stale_v is None:
        a, b = dense(case, t)[0], dense(case, t, part=128)[0]
        assert float((a - b).abs().max()) <= 1e-9


def rope_kw(case, t, stale=False):
    """``dense`` arguments of a RoPE case's row: the q the kernel sees after its rotation, and the new
    token's V from the qkv row (or, the mistake, the stale cache slot's)."""
    if case.stale_v is None:
        return {}
    c, si = int(case.q_ctx[t]), int(case.q_seq[t])
    q = case.q[t].double().view(-1, case.D)[: case.nh]
    if float(case.cos[0, 0]) == 0.0:  # quarter turn: rotate_half with cos 0, sin 1
        h = case.D // 2
        q = torch.cat([-q[:, h:], q[:, :h]], -1)
    return dict(q=q, v_override=(c - 1, case.stale_v[si] if stale else case.seqs[si].V[:, c - 1]))


@pytest.mark.parametrize("nh,nkv,D", DECODE_SHAPES)
def test_decode_case_covers_every_edge_and_is_exact(nh, nkv, D):
    case = _decode(nh, nkv, D)
    assert case.q.dtype == torch.bfloat16 and case.k_cache.dtype == torch.bfloat16
    kf, vf = case.f8()  # asserts the exact fp8 round trip of K and V
    assert int((kf.codes == 0xFF).all(-1).sum()) == int(case.poison.sum()) * nkv
    parts = ap.decode_partitions(case.T, nkv, max(ap.DECODE_CTXS))
    assert len(parts) >= 4
    if nh * (case.T // len(ap.DECODE_CTXS)) >= 48:  # enough (row, head) slots: every edge has a single probe
        for seq, n in zip(case.seqs, ap.DECODE_CTXS):
            aimed = {pr.a for t in seq.rows for pr in case.probes[t] if pr.kind == "single"}
            assert aimed == set(ap.decode_edges(n, D, sorted({p for p, _ in parts})))
    else:  # few heads: the plain and the ctx-below-cache case cover every edge between them
        short = _decode(nh, nkv, D, True)
        for i, n in enumerate(ap.DECODE_CTXS):
            aimed = {pr.a for c in (case, short) for t in c.seqs[i].rows for pr in c.probes[t] if pr.kind == "single"}
            assert aimed == set(ap.decode_edges(n, D, sorted({p for p, _ in parts})))
    # the block table names valid pages only, and what follows the trap is NaN
    assert int(case.block_tables.min()) >= 0 and int(case.block_tables.max()) < case.k_cache.shape[0]
    for seq in case.seqs:
        assert seq.K[seq.N + 1 :].isnan().all() and seq.K[-64:].isnan().all() and seq.K.shape[0] - seq.N - 1 >= 64
        assert torch.isfinite(seq.K[: seq.N + 1]).all()


@pytest.mark.parametrize("nh,nkv,D", DECODE_SHAPES)
@pytest.mark.parametrize("f8", [False, True])
def test_reference_op_passes_comparator_decode(nh, nkv, D, f8):
    for short in (False, True):
        case = _decode(nh, nkv, D, short)
        a = case.to("cpu")
        kc, vc = case.f8() if f8 else (a["k_cache"], a["v_cache"])
        out = ops.paged_attention(a["q"], kc, vc, a["block_tables"], a["q_seq"], a["q_ctx"], nh, nkv, case.scale)
        assert ap.compare(out, case, "reference") <= 2.0 ** -8


@pytest.mark.parametrize("op", ["mfma", "fa"])
def test_reference_op_passes_comparator_prefill(op):
    nh, nkv, D = 16, 4, 128
    case = _prefill(nh, nkv, D)
    a = case.to("cpu")
    args = (a["q"], a["k_cache"], a["v_cache"], a["block_tables"], a["q_seq"], a["q_ctx"])
    nt = ap.qctx_lists(case)
    if op == "mfma":
        out = ops.attention_mfma(*args, torch.from_numpy(ops.query_blocks(nt, nh // nkv)), nh, nkv, case.scale)
    else:
        out = ops.attention_fa(*args, torch.from_numpy(ops.fa_blocks(nt, nh // nkv)), nh, nkv, case.scale)
    assert ap.compare(out, case, op) <= 2.0 ** -8
    assert int(case.probe_rows.sum()) >= 10 and not bool(case.probe_rows.all())


@pytest.mark.parametrize("quarter", [False, True])
@pytest.mark.parametrize("f8", [False, True])
def test_reference_op_passes_comparator_rope(quarter, f8):
    nh, nkv, D = 12, 12, 64
    case = _rope(nh, nkv, D, quarter)
    a = case.to("cpu")
    kc, vc = case.f8() if f8 else (a["k_cache"], a["v_cache"])
    out = ops.paged_attention_rope(a["q"], kc, vc, a["block_tables"], a["q_seq"], a["q_ctx"], a["positions"],
                                   a["cos"], a["sin"], a["slots"], nh, nkv, case.scale)
    ap.compare(out, case, "rope reference")
    assert torch.equal(a["q"], case.q)
    ka, va = (kc.dequant(), vc.dequant()) if f8 else (kc, vc)
    ok = ~case.poison[:, None, :, None].expand_as(ka)
    assert torch.equal(ka[ok], case.k_after[ok]) and torch.equal(va[ok], case.v_after[ok])
    assert ka[~ok].isnan().all() and va[~ok].isnan().all()


# ---- mutations: the comparator must reject every probe row that depends on the mistake ----------
MUT_CASES = ["decode-32-8-128", "decode-12-12-64", "prefill-12-12-64"]


def test_unmutated_reference_passes():
    for mk in MUT_CASES:
        case = CASES[mk]()
        assert ap.compare(mutated(case, probe_rows(case)), case) <= 2.0 ** -8


@pytest.mark.parametrize("mk", MUT_CASES)
def test_mutation_dropped_key_at_each_edge(mk):
    case = CASES[mk]()
    n = 0
    for seq in case.seqs:
        rows = [t for t in seq.rows if case.probes[t] is not None]
        for e in sorted({k for t in rows for pr in case.probes[t] for k in pr.keys}):
            hit_rows = [t for t in rows if any(e in pr.keys for pr in case.probes[t])]
            out = mutated(case, hit_rows, drop=(e,))
            n += assert_rejects(case, out, lambda t, pr: t in hit_rows and e in pr.keys, f"dropped key {e}")
    assert n >= case.nh * len(probe_rows(case))  # every probe depends on at least one key


@pytest.mark.parametrize("mk", MUT_CASES)
def test_mutation_visible_trap(mk):
    case = CASES[mk]()
    out = mutated(case, probe_rows(case), trap=True)
    assert assert_rejects(case, out, lambda t, pr: pr.kind == "single", "visible trap") > 0


@pytest.mark.parametrize("mk", MUT_CASES)
def test_mutation_last_key_counted_twice(mk):
    case = CASES[mk]()
    rows = [t for t in probe_rows(case) if int(case.q_ctx[t]) >= 2]
    out = case.expected.clone().view(case.T, case.nh, case.D)
    for t in rows:
        out[t] = dense(case, t, twice=int(case.q_ctx[t]) - 1)[0]
    out = out.view(case.T, -1).to(torch.bfloat16)
    hit = lambda t, pr: t in rows and pr.kind != "single" and int(case.q_ctx[t]) - 1 in pr.keys
    assert assert_rejects(case, out, hit, "last key counted twice") > 0


@pytest.mark.parametrize("mk", MUT_CASES)
@pytest.mark.parametrize("part", [64, 128, 256, 2048])
def test_mutation_slice_partial_left_out(mk, part):
    case = CASES[mk]()
    n = 0
    for t in probe_rows(case):
        for sl in sorted({k // part for pr in case.probes[t] for k in pr.keys}):
            out = mutated(case, [t], part=part, skip=sl)
            n += assert_rejects(case, out, lambda tt, pr: tt == t and any(k // part == sl for k in pr.keys),
                                f"slice {sl} of {part} left out")
    assert n > 0


@pytest.mark.parametrize("mk", ["rope-32-8-128", "rope-quarter-12-12-64"])
def test_mutation_stale_slot_used_for_new_token(mk):
    case = CASES[mk]()
    out = case.expected.clone().view(case.T, case.nh, case.D)
    for t in range(case.T):
        out[t] = dense(case, t, **rope_kw(case, t, stale=True))[0]
    out = out.view(case.T, -1).to(torch.bfloat16)
    n = assert_rejects(case, out, lambda t, pr: int(case.q_ctx[t]) - 1 in pr.keys, "stale slot")
    assert n == case.nh * case.T  # every RoPE probe depends on the new token
