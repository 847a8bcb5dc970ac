"""Sliding-window PREFILL probes: the closed-form probes of ``tests/attn_probe.py`` for chunks whose rows
have different contexts, under a window (plain module, CPU only).  Page 64, D = 128, Hadamard special
keys, ``attn_probe.compare`` and its derived bound 2^-6.

With a window W a row of context c sees ``[lo, c)``, ``lo = max(0, c - W)``.  The windowed FA2 kernel
(csrc/attention_fa.hip WIN form) streams a block from ``base = lo(first row) & ~63`` in 64-token steps
and places slice p of a split launch at ``base + p PS``: every slice edge is a 64-token step edge.

Probes of a probe row:

* singles at ``lo``, ``lo + 1`` and ``c - 1``; pairs and weighted pairs ``(lo, c - 1)`` and ``(lo, lo + 1)``;
* singles and pairs across every 64-token step edge x with ``lo < x < c`` (positions x - 1 and x) - these
  are the slice edges ``base + k PS`` for PS in 64 / 128 / 256 too;
* the lower trap, on rows with ``lo - 1`` at or above the sequence's first row's ``lo``: position
  ``lo - 1`` is another row's visible key, so it cannot be NaN.  The query is ``g (K[lo] + K[lo - 1])``
  and its expected output under the window is ``V[lo]`` alone; a kernel that reads ``lo - 1`` returns the
  mean of the two special V rows, which differ by >= 0.5 in >= D/4 channels: off by >= 0.25.  The builder
  sees that query as the pair ``(lo - 1, lo)``; ``prefill_window_case`` puts the expected row right.
* the upper trap is the builder's: a Hadamard row at c (the chunk's next token) and NaN after the last.

Poison from below: every position below the sequence's FIRST query row's ``lo`` is NaN (0xFF codes and
scales in an fp8 cache), and the block-table entries of the pages wholly below it name the all-NaN valid
page - what ``attn_window_probe._poison_below`` does for rows of one context.

A sequence has at most D - 1 = 127 special positions (the builder asserts it): probe ROWS are taken in
order of priority while they fit, probe kinds are never dropped.
"""
from typing import List, Sequence, Tuple

import torch

from tests import attn_probe as ap
from tests.attn_window_probe import lo_of

WINDOWS = (1, 33, 64, 100)
PARTS = (64, 128, 256)
STEP = 64
D = 128

# (tokens, prefix) of the sequences of one launch
SEQS = ((130, 0),           # lo goes from 0 to positive inside the chunk
        (70, 200),          # a chunk wholly past the window ...
        (40, 0))            # ... next to one wholly inside it (W >= 40) or crossing it
# nh = nkv = 4 only: a 4-wave block holds 128 tokens and an 8-wave block 256, so at W = 1 and 33 a
# block's last rows have their lo one and two (and more) 64-token steps above base: real rows that are
# fully masked in the first steps their wave computes
SEQ_MHA = (200, 60)


def seqs_of(nh: int, nkv: int) -> Tuple[Tuple[int, int], ...]:
    return SEQS + ((SEQ_MHA,) if nh == nkv else ())


def _row_probes(c: int, W: int, lo_first: int):
    """(fixed, cycle, lowtrap) of a row of context c: ``fixed`` sits on the first heads of the row."""
    lo = lo_of(c, W)
    vis = lambda *xs: all(lo <= x < c for x in xs) and len(set(xs)) == len(xs)  # noqa: E731
    trap = lo - 1 >= lo_first and lo >= 1
    singles = [lo, c - 1, lo + 1]
    pairs = [(lo, c - 1), (lo, lo + 1)]
    for x in range(STEP * (lo // STEP + 1), c, STEP):  # step edges: x - 1 and x both visible
        if vis(x - 1, x):
            singles += [x, x - 1]
            pairs.append((x - 1, x))
    singles = [x for x in dict.fromkeys(singles) if vis(x)]
    pairs = [p for p in dict.fromkeys(pairs) if p[0] < p[1] and vis(*p)]
    # the lower trap stands in the builder as the pair (lo - 1, lo): the same query
    fixed = [ap.Probe("pair", lo - 1, lo)] if trap else [ap.Probe("single", lo)]
    if c - 1 != lo:
        fixed.append(ap.Probe("single", c - 1))
    cyc = [ap.Probe("single", x) for x in singles if x != c - 1 and (trap or x != lo)]
    cyc += [ap.Probe("pair", a, b) for a, b in pairs]
    cyc += [ap.Probe("weighted", a, b) for a, b in pairs[:2]] + [ap.Probe("weighted", b, a) for a, b in pairs[:2]]
    return fixed, cyc, trap


def probe_rows(n: int, pre: int, W: int, nrep: int) -> List[int]:
    """Row indices of a chunk in order of priority: the ends, the rows where ``lo`` leaves 0, where
    ``lo`` or the context crosses a 64-token step, and the wave / block edges (32 / nrep tokens a wave)."""
    tpw = max(1, 32 // nrep)
    ctxs = [W, W + 1, W + 2]
    for x in range(STEP, pre + n + STEP, STEP):
        ctxs += [x + W, x + W + 1, x + W - 1, x, x + 1]
    rows = [n - 1, 0, 4 * tpw - 1, 4 * tpw, 8 * tpw - 1, 8 * tpw] + [c - pre - 1 for c in ctxs]
    rows += [tpw - 1, tpw, 2 * tpw - 1, 2 * tpw]
    return [j for j in dict.fromkeys(rows) if 0 <= j < n]


def prefill_window_case(nh: int, nkv: int, W: int, seqs: Sequence[Tuple[int, int]] = None, seed: int = 0) -> ap.Case:
    """One launch of chunked causal prefill under window ``W``: sequence i has ``prefix`` cached tokens and
    ``n`` query rows (row j: context prefix + j + 1), poisoned below its first row's ``lo``."""
    seqs = seqs_of(nh, nkv) if seqs is None else seqs
    rep = nh // nkv
    specs, traps = [], []
    for n, pre in seqs:
        N = pre + n
        lo_first = lo_of(pre + 1, W)
        sp, chosen = {N}, {}
        for j in probe_rows(n, pre, W, rep):
            c = pre + j + 1
            fixed, cyc, trap = _row_probes(c, W, lo_first)
            need = {k for p in fixed + cyc for k in p.keys} | {c}
            if len(sp | need) > D - 1:
                continue  # the budget of special positions: this row is dropped, no probe kind is
            sp |= need
            chosen[j] = (ap._heads(nh, len(chosen), cyc, fixed), trap)
        assert n - 1 in chosen and 0 in chosen and min(sp) >= lo_first
        specs.append((N, sp, [(pre + j + 1, chosen[j][0] if j in chosen else None) for j in range(n)]))
        traps.append({j for j, (_, t) in chosen.items() if t})
    case = ap._build(nh, nkv, D, specs, seed)
    exp = case.expected.view(case.T, nh, D)
    for (n, pre), seq, tr in zip(seqs, case.seqs, traps):
        for j in tr:
            t, lo = seq.rows[j], lo_of(pre + j + 1, W)
            assert case.probes[t][0] == ap.Probe("pair", lo - 1, lo)
            for h, pr in enumerate(case.probes[t]):
                if pr == ap.Probe("pair", lo - 1, lo):  # the lower trap: V[lo] alone
                    exp[t, h] = seq.V[h // rep, lo]
                    case.probes[t][h] = ap.Probe("lowtrap", lo, lo - 1)
    _poison_below_first(case, W)
    return case


def _poison_below_first(case: ap.Case, W: int) -> None:
    """NaN below every sequence's first row's ``lo``; block-table entries of the pages wholly below it ->
    the all-NaN valid page."""
    held = {pg for s in case.seqs for pg in s.pages}
    free = [pg for pg in range(case.k_cache.shape[0]) if pg not in held and bool(case.poison[pg].all())]
    assert free, "the builder leaves all-NaN pages no sequence holds"
    for si, seq in enumerate(case.seqs):
        lo = lo_of(int(case.q_ctx[seq.rows[0]]), W)
        seq.K[:lo] = float("nan")
        seq.V[:, :lo] = float("nan")
        for j, pg in enumerate(seq.pages):
            n = min(max(lo - j * ap.PAGE, 0), ap.PAGE)  # positions of this page below lo
            case.k_cache[pg, :, :n] = float("nan")
            case.v_cache[pg, :, :n] = float("nan")
            if n == ap.PAGE:
                case.block_tables[si, j] = free[0]
    case.poison = case.k_cache[:, 0, :, 0].isnan()
    assert torch.equal(case.poison, case.v_cache[:, 0, :, 0].isnan())
    assert not case.expected.isnan().any() and not case.q.isnan().any()


def ntoks(case: ap.Case) -> List[int]:
    return ap.qctx_lists(case)


def block_tokens(nh: int, nkv: int, waves: int) -> int:
    """BT: the most tokens an FA2 block holds."""
    return max(1, (32 * waves) // (nh // nkv))


def span(case: ap.Case, W: int, waves: int) -> int:
    """Tokens the wrapper's slices must cover: ``min(max_ctx, W + BT + 62)``."""
    return min(int(case.q_ctx.max()), W + block_tokens(case.nh, case.nkv, waves) + 62)


def partitions(case: ap.Case, W: int, waves: int):
    """(part_size, num_parts) of the explicit launches: 64 / 128 / 256-token slices, enough of them to
    cover the streamed span plus two that stay empty in every block."""
    s = span(case, W, waves)
    return [(ps, -(-s // ps) + 2) for ps in PARTS]
