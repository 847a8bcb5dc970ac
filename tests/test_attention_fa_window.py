"""The windowed FA2 prefill ops off the GPU: the prefill window probes are consistent (the fp32 reference
passes them at 2^-6 and a reference that reads one key too many does not), ``ops.attention_fa_window``
on CPU tensors is ``ops.paged_attention(window=)``, its argument checks, and the span its slices cover."""
import functools
import math

import pytest
import torch

from src import ops
from src.ops import reference as ref
from tests import attn_probe as ap
from tests import attn_window_prefill_probe as pp

SHAPES = [(4, 4), (4, 2), (8, 2), (8, 1)]


@functools.lru_cache(maxsize=None)
def _case(nh, nkv, W):
    return pp.prefill_window_case(nh, nkv, W)


def _ref_args(case):
    return (case.q.float(), case.k_cache.float(), case.v_cache.float(), case.block_tables, case.q_seq, case.q_ctx)


@pytest.mark.parametrize("nh,nkv", SHAPES)
@pytest.mark.parametrize("W", pp.WINDOWS)
def test_the_reference_passes_the_prefill_window_probes(nh, nkv, W):
    case = _case(nh, nkv, W)
    a = _ref_args(case)
    ap.compare(ref.paged_attention(*a, nh, nkv, case.scale, window=W), case, f"reference W={W}")
    kf, vf = case.f8()
    ap.compare(ref.paged_attention_f8(a[0], kf, vf, *a[3:], nh, nkv, case.scale, window=W), case, f"reference f8 W={W}")


@pytest.mark.parametrize("W", pp.WINDOWS)
def test_the_prefill_window_probes_can_tell(W):
    """One key too many below ``lo`` (window W + 1): the first rows of a chunk past the window meet NaN,
    and every lower-trap row is off by >= 0.25.  No window at all: NaN.  The cases hold what they claim."""
    nh, nkv = 4, 4
    case = _case(nh, nkv, W)
    a = _ref_args(case)
    for wide in (W + 1, 0):
        with pytest.raises(AssertionError, match="non-finite"):
            ap.compare(ref.paged_attention(*a, nh, nkv, case.scale, window=wide), case)
    # the lower trap alone: the poison taken out, a reference that reads lo - 1 is rejected on those rows
    kc, vc = torch.nan_to_num(a[1]), torch.nan_to_num(a[2])
    out = ref.paged_attention(a[0], kc, vc, *a[3:], nh, nkv, case.scale, window=W + 1)
    dev = ap.deviation(out, case)
    traps = [(t, h) for t, pl in enumerate(case.probes) if pl for h, p in enumerate(pl) if p.kind == "lowtrap"]
    assert len(traps) >= 8
    for t, h in traps:
        assert float(dev[t, h]) >= 0.25, (t, h, float(dev[t, h]))
    # probed: lo, lo + 1 and c - 1 of rows past the window, both sides of a 64-token step edge, all kinds
    kinds, keys = set(), set()
    for t, pl in enumerate(case.probes):
        for p in pl or ():
            c = int(case.q_ctx[t])
            lo = pp.lo_of(c, W)
            kinds.add(p.kind)
            keys |= {("lo", lo > 0) for k in p.keys if k == lo} | {("diag",) for k in p.keys if k == c - 1}
            if p.kind == "pair" and p.b % 64 == 0 and p.a == p.b - 1:
                keys.add(("edge",))
    assert kinds >= {"single", "lowtrap"} and keys >= {("lo", True), ("lo", False), ("diag",)}
    assert W == 1 or (kinds >= {"pair", "weighted"} and ("edge",) in keys)  # (W = 1: one visible key, no pairs)
    # poison from below: a chunk past the window has NaN below its first lo and all-NaN pages below that
    for si, (n, pre) in enumerate(pp.seqs_of(nh, nkv)):
        lo = pp.lo_of(pre + 1, W)
        assert case.seqs[si].K[:lo].isnan().all() and not case.seqs[si].K[lo:pre + n + 1].isnan().any()
        for j in range(lo // 64):
            assert bool(case.poison[int(case.block_tables[si, j])].all())
    # the fully-masked-first-steps case: the 4 / 8-wave blocks of the 200-token chunk hold probe rows whose
    # lo lies at least one / two 64-token steps above the block's base
    if W in (1, 33):
        n, pre = pp.SEQ_MHA
        seq = case.seqs[-1]
        for bt_ in (128, 256):
            above = set()
            for j in range(n):
                if case.probes[seq.rows[j]] is not None:
                    base = pp.lo_of(pre + (j // bt_) * bt_ + 1, W) & ~63
                    above.add((pp.lo_of(pre + j + 1, W) - base) // 64)
            assert above >= {0, 1, 2}, (bt_, above)


def test_attention_fa_window_on_cpu_is_the_windowed_reference():
    nh, nkv, W = 8, 2, 33
    case = _case(nh, nkv, W)
    a = _ref_args(case)
    fb = torch.from_numpy(ops.fa_blocks(pp.ntoks(case), nh // nkv, 4))
    q = a[0][:, : nh * pp.D].contiguous()
    want = ops.paged_attention(q, *a[1:], nh, nkv, case.scale, window=W)
    got = ops.attention_fa_window(q, *a[1:], fb, nh, nkv, case.scale, W)
    assert torch.equal(got, want)
    ap.compare(got, case, "attention_fa_window on the CPU")
    assert not torch.equal(torch.nan_to_num(ops.paged_attention(q, *a[1:], nh, nkv, case.scale)), want)
    kf, vf = case.f8()
    got8 = ops.attention_fa_window_f8(q, kf, vf, *a[3:], fb, nh, nkv, case.scale, W)
    ap.compare(got8, case, "attention_fa_window_f8 on the CPU")
    with pytest.raises(TypeError):
        ops.attention_fa_window_f8(q, *a[1:], fb, nh, nkv, case.scale, W)
    with pytest.raises(NotImplementedError, match="fp8 KV"):
        ops.attention_fa_window(q, kf, vf, *a[3:], fb, nh, nkv, case.scale, W)


def test_attention_fa_window_argument_checks():
    nh, nkv, W = 4, 4, 64
    case = _case(nh, nkv, W)
    a = _ref_args(case)
    fb = torch.from_numpy(ops.fa_blocks(pp.ntoks(case), 1, 4))
    q = a[0][:, : nh * pp.D].contiguous()
    for bad in (0, -1):
        with pytest.raises(ValueError, match="window"):
            ops.attention_fa_window(q, *a[1:], fb, nh, nkv, case.scale, bad)
        with pytest.raises(ValueError, match="window"):
            ops.attention_fa_window_f8(q, *case.f8(), *a[3:], fb, nh, nkv, case.scale, bad)
    # explicit slices must cover _window_span(W, max_ctx, BT + 62); BT = 128 tokens at 4 waves, HB 1
    mc = int(case.q_ctx.max())
    span = ops._window_span(W, mc, 128 + 62)
    assert span == min(mc, W + 190) == 254 and ops.fa_window_pad(nh, nkv, 4) == 190 and ops.fa_window_pad(8, 1, 8) == 94
    with pytest.raises(ValueError, match="cover"):
        ops.attention_fa_window(q, *a[1:], fb, nh, nkv, case.scale, W, max_ctx=mc, waves=4, part_size=64, num_parts=3)
    with pytest.raises(ValueError, match="cover"):  # 8 waves: BT = 256
        ops.attention_fa_window(q, *a[1:], fb, nh, nkv, case.scale, W, max_ctx=mc, waves=8, part_size=128, num_parts=1)
    with pytest.raises(ValueError, match="part_size"):
        ops.attention_fa_window(q, *a[1:], fb, nh, nkv, case.scale, W, max_ctx=mc, part_size=96, num_parts=8)
    with pytest.raises(ValueError, match="part_size"):
        ops.attention_fa_window(q, *a[1:], fb, nh, nkv, case.scale, W, max_ctx=mc, part_size=64)
    ops.attention_fa_window(q, *a[1:], fb, nh, nkv, case.scale, W, max_ctx=mc, waves=4, part_size=64, num_parts=4)


@pytest.mark.parametrize("W", pp.WINDOWS)
def test_the_span_bound_against_brute_force(W):
    """A block of n consecutive tokens with first context c streams c + n - 1 - (max(0, c - W) & ~63)
    tokens: never more than _window_span(W, max_ctx, BT + 62), and the bound is reached."""
    for nrep, waves in ((1, 4), (1, 8), (2, 4), (4, 8), (8, 4), (8, 8)):
        BT = max(1, 32 * waves // nrep)
        assert ops.fa_window_pad(8, 8 // nrep, waves) == BT + 62
        worst = 0
        for c in range(1, 401):
            base = max(0, c - W) & ~63
            for n in range(1, BT + 1):
                streamed = c + n - 1 - base
                assert streamed <= ops._window_span(W, c + n - 1, BT + 62)
                worst = max(worst, streamed)
        assert worst == W + BT + 62
