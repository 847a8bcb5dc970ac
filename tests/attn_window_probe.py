"""Sliding-window probes: the closed-form attention probes of ``tests/attn_probe.py`` with a lower bound
on the keys (plain module, CPU only).

With a window W a query of context ``ctx`` sees cache positions ``[lo, ctx)``, ``lo = max(0, ctx - W)``.
A case is built by the existing builder from probes whose keys all lie in ``[lo, ctx)`` and is then
poisoned from below:

* every cache position below a row's ``lo`` holds NaN (0xFF in the codes and scales of an fp8 cache) -
  the positions of the retained page below ``lo`` and those of the first 32-token step included;
* the block-table entries of the pages wholly below ``lo`` name the all-NaN VALID page, as released
  entries would name no page at all: a kernel that looks one up reads NaN, never unmapped memory.

NaN is the lower trap: a kernel that reads one key too many returns a non-finite row, which
``attn_probe.compare`` rejects (the upper trap stays the builder's: the Hadamard row at ``ctx`` and
NaN after it).  Probes, per context: singles at ``lo`` and ``lo + 1``, pairs and weighted pairs
``(lo, ctx - 1)`` and ``(lo, lo + 1)``, the decode edge probes of ``attn_probe`` that fall into
``[lo, ctx)``, and singles and pairs across every slice boundary as the kernel places it:
``lo + k PS`` (flash-decoding) or ``(lo & ~31) + k PS`` (MFMA), PS in 64 / 128 / 256.
The comparator and its derived bound 2^-6 are ``attn_probe.compare``'s.
"""
import math
from typing import List

import torch

from src import ops
from tests import attn_probe as ap

WINDOWS = (1, 33, 64, 100)
FD_PARTS = (64, 128, 256)    # slice sizes probed on the flash-decoding kernel
MFMA_PARTS = (128, 256)      # ... and on the MFMA kernel (slices of a multiple of 128 tokens)


def window_ctxs(W: int) -> List[int]:
    """Contexts of one launch: ``lo`` at 0, 1 and each side of a 32-token step and of a page."""
    cs = (1, W - 1, W, W + 1, W + 31, W + 32, W + 33, W + 64, 2 * W + 65, W + 1000)
    return [c for c in dict.fromkeys(cs) if c >= 1]


def lo_of(ctx: int, W: int) -> int:
    return max(0, ctx - W) if W else 0


def slice_base(ctx: int, W: int, mfma: bool) -> int:
    """First position of slice 0 as the kernel places it."""
    lo = lo_of(ctx, W)
    return lo & ~31 if mfma else lo


def span(max_ctx: int, W: int, mfma: bool) -> int:
    """Tokens per query a windowed launch streams (what its slices must cover)."""
    return min(max_ctx, W + (31 if mfma else 0))


def _window_probes(n: int, W: int, D: int, mfma: bool, rope: bool) -> List[ap.Probe]:
    lo = lo_of(n, W)
    parts = MFMA_PARTS if mfma else FD_PARTS
    base = slice_base(n, W, mfma)
    vis = lambda *xs: all(lo <= x < n for x in xs)  # noqa: E731
    pairs = [(lo, n - 1), (lo, lo + 1), (n - 2, n - 1)]
    singles = [n - 1, lo, lo + 1] if rope else [lo, lo + 1, n - 1]
    for ps in parts:
        for k in range(1, (n - base) // ps + 1):
            x = base + k * ps
            pairs.append((x - 1, x))
            singles += [x, x - 1, x + 1]
    singles += [x for x in ap.decode_edges(n, D, parts) if x >= lo]
    pairs = [(a, b) for a, b in dict.fromkeys(pairs) if a < b and vis(a, b)]
    singles = [x for x in dict.fromkeys(singles) if vis(x)]
    if rope:  # one row per sequence: the probes that involve the new token n - 1 and lo come first
        out = [ap.Probe("single", n - 1)]
        for a, b in pairs[:1]:
            out += [ap.Probe("pair", a, b), ap.Probe("weighted", a, b), ap.Probe("weighted", b, a)]
        out += [ap.Probe("single", x) for x in singles[1:3]]
        out += [ap.Probe("pair", a, b) for a, b in pairs[1:]]
        return out + [ap.Probe("single", x) for x in singles[3:]]
    out = [ap.Probe("single", x) for x in singles[:2]]
    out += [ap.Probe("pair", a, b) for a, b in pairs]
    out += [ap.Probe("weighted", a, b) for a, b in pairs[:2]] + [ap.Probe("weighted", b, a) for a, b in pairs[:2]]
    return out + [ap.Probe("single", x) for x in singles[2:]]


def _poison_below(case: ap.Case, W: int) -> None:
    """NaN below every sequence's ``lo``; block-table entries of the pages wholly below it -> the all-NaN page."""
    held = {pg for s in case.seqs for pg in s.pages}
    free = [pg for pg in range(case.k_cache.shape[0]) if pg not in held and bool(case.poison[pg].all())]
    assert free, "the builder leaves all-NaN pages no sequence holds"
    nan_page = free[0]
    for si, seq in enumerate(case.seqs):
        ctxs = {int(case.q_ctx[t]) for t in seq.rows}
        assert len(ctxs) == 1, "every row of a window sequence has the same context"
        lo = lo_of(ctxs.pop(), W)
        seq.K[:lo] = float("nan")
        seq.V[:, :lo] = float("nan")
        for j, pg in enumerate(seq.pages):
            n = min(max(lo - j * ap.PAGE, 0), ap.PAGE)  # positions of this page below lo
            for c in (case.k_cache, case.v_cache, case.k_after, case.v_after):
                if c is not None:
                    c[pg, :, :n] = float("nan")
            if n == ap.PAGE:
                case.block_tables[si, j] = nan_page
    case.poison = case.k_cache[:, 0, :, 0].isnan()
    assert torch.equal(case.poison, case.v_cache[:, 0, :, 0].isnan())
    assert not case.expected.isnan().any()


def window_case(nh, nkv, D, W, mfma=False, seed=0) -> ap.Case:
    """One decode launch under window ``W``: a sequence per context of ``window_ctxs``, up to 4 query
    rows each (q_ctx = n), every (row, head) another probe; poisoned below ``lo``."""
    specs = []
    for n in window_ctxs(W):
        pl = _window_probes(n, W, D, mfma, False)
        rows = min(4, math.ceil(len(pl) / nh))
        sp = {k for p in pl[: rows * nh] for k in p.keys} | {n}
        specs.append((n, sp, [(n, ap._heads(nh, j, pl)) for j in range(rows)]))
    case = ap._build(nh, nkv, D, specs, seed)
    _poison_below(case, W)
    return case


def window_rope_case(nh, nkv, D, W, mfma=False, quarter=False, seed=0) -> ap.Case:
    """A RoPE-fused decode step under window ``W`` (``attn_probe.rope_case``'s construction: the qkv row
    carries the new token's k and v, its slot holds a stale trap, identity or quarter-turn rotary
    table), one query per context of ``window_ctxs``; poisoned below ``lo``."""
    ctxs = window_ctxs(W)
    specs = []
    for n in ctxs:
        pl = _window_probes(n, W, D, mfma, True)[:nh]
        specs.append((n, {k for p in pl for k in p.keys} | {n}, [(n, ap._heads(nh, 0, pl))]))
    case = ap._build(nh, nkv, D, specs, seed)
    gen = torch.Generator().manual_seed(seed + 1)
    T = case.T
    qkv = case.q.double().view(T, nh + 2 * nkv, D).clone()
    case.k_after, case.v_after = case.k_cache.clone(), case.v_cache.clone()
    case.stale_v, slots = [], []
    for t, (seq, n) in enumerate(zip(case.seqs, ctxs)):
        qkv[t, nh: nh + nkv] = seq.K[n - 1]
        qkv[t, nh + nkv:] = seq.V[:, n - 1]
        while True:
            stale = torch.randint(-4, 5, (nkv, D), generator=gen).double() * 0.5
            if int((stale != seq.V[:, n - 1]).sum(-1).min()) >= D // 4:
                break
        case.stale_v.append(stale)
        pg, off = seq.pages[(n - 1) // ap.PAGE], (n - 1) % ap.PAGE
        case.v_cache[pg, :, off] = stale.to(ap.BF)
        slots.append(pg * ap.PAGE + off)
    if quarter:
        qkv[:, : nh + nkv] = ap._unrotate_quarter(qkv[:, : nh + nkv])
    case.q = ap._exact_bf16(qkv.reshape(T, -1))
    case.positions = case.q_ctx.long() - 1
    case.slots = torch.tensor(slots, dtype=torch.int64)
    tab = torch.zeros(max(ctxs) + 1, D // 2, dtype=torch.float32)
    case.cos, case.sin = (tab, tab + 1) if quarter else (tab + 1, tab)
    _poison_below(case, W)
    return case


def window_partitions(case: ap.Case, W: int, mfma: bool):
    """(part_size, num_parts) of the explicit launches: 64 / 128 / 256-token slices (128 / 256 on the
    MFMA kernel), enough of them to cover the streamed span plus two that stay empty."""
    s = span(int(case.q_ctx.max()), W, mfma)
    return [(ps, math.ceil(s / ps) + 2) for ps in (MFMA_PARTS if mfma else FD_PARTS)]


def default_part_size(case: ap.Case, W: int, mfma: bool, rope: bool) -> int:
    """The slice size the wrapper picks itself; the probes cover its boundaries only if it is a probed one."""
    s = span(int(case.q_ctx.max()), W, mfma)
    if not mfma:
        return ops.attention_partition(case.T, case.nkv, s)[0]
    if rope:
        return 128 * math.ceil(s / 128)
    return ops._mfma_partition(case.T, case.nh, case.nkv, s)[0]


def check_cache_after(case: ap.Case, kc, vc, f8: bool) -> None:
    """After a RoPE-fused launch: the new token's slot holds the new k / v bit for bit, every other
    slot is unchanged and every poisoned slot is still poison."""
    ka, va = (kc.dequant(), vc.dequant()) if f8 else (kc, vc)
    ok = ~case.poison[:, None, :, None].expand_as(case.k_after)
    for got, want, name in ((ka.cpu(), case.k_after, "k"), (va.cpu(), case.v_after, "v")):
        assert torch.equal(got[ok], want[ok]), f"{name} cache after the launch"
        assert got[~ok].isnan().all(), f"{name} cache: a poisoned slot was written"
    if f8:
        pz = case.poison[:, None, :].expand_as(kc.scales.cpu())
        for c in (kc, vc):
            assert (c.codes.cpu()[pz] == 0xFF).all() and (c.scales.cpu()[pz] == 0xFF).all()
